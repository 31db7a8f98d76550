// repair_remote.hip — rewriting damaged replica logs from a peer over the transport
// (rmq_repair_remote, FORMAT.md §10 "Remote repair"), gfx950.
//
// The first pass is rmq_repair's (repair.hip): the plan, a verdict per task, the local copy. What it
// leaves failing with no passing local slot is asked of the ranks that hold the partition's other
// replica slots, one candidate rank per round. Three kernels serve a round:
//   request  the requester's lanes over the tasks of the plan, as repair_copy_kernel takes them: a
//            pair still wanted whose segment has bounds and ends at or below this replica's commit
//            is appended to the list of the round's candidate rank;
//   serve    the donor, one wave per request received: the checks, the walk of the span in its own
//            ring (serve_check), then the header, the directory and a 64 lanes x 16 B copy of each
//            passing span to the place a prefix over the accepted spans gives it (serve_copy);
//   install  the requester, one wave per directory entry received: the structure, the walk of the
//            span in the inbox, and only then the copy into the failing slot's ring.
//
// Bounds. No word that crossed the transport is an address or a loop bound.
//   request: a request slot is the value of the destination's counter, used only below max_reqs,
//     which is what one list holds (list_cap = kRemoteHdr + max_reqs * kRemoteReq); the destination
//     is a rank of the host's candidate table, used only below world.
//   serve: the number of requests of a source is what the host derived from the bytes it received,
//     never the list header's count. key is only compared (binary search over nkeys entries); the
//     pidx comes from the donor's own table. pos, end, expect and eoff are used only after
//     log_start_pos <= pos < end <= log_end_pos, (pos | end) & 15 == 0, end - pos <= S_p and
//     log_start_offset <= expect <= eoff <= min(log_end_offset, commit) against the donor's own
//     state of a sane log (scrub_part); every ring read is masked with the donor's S_p - 1. The
//     walk is bounded by end: a record is at least 16 bytes, and its piece count is clamped by the
//     pieces left in the span before any payload piece is loaded. The output position of a span is
//     the sum of the span bytes the check kernel accepted before it (chunk sums and the verdict
//     words of its own chunk), and the host sized the response from their total; cookie is echoed,
//     never used.
//   install: the entries of a rank are the requests this rank sent it (w0), the cookie must equal
//     the one of the same slot of the list as sent, and the task, its ring, pos, end, expect and
//     eoff are decoded again from the rank's own plan (scrub_task): the span's size is end - pos of
//     that task. data_start comes from the response and is used only after data_start + (end - pos)
//     <= the response's data bytes, which the header must state as exactly the bytes received
//     minus header and directory; an entry is accepted only where the directory tiles the data
//     section (entry 0 at 0, the next entry, or the section's end, exactly behind it). The walk of
//     the inbox span is bounded as the serve's; the ring stores are masked with the requester's own
//     S_p - 1. A pair is written at most once: its want byte is cleared by the wave that heals it,
//     and a task is in at most one list per round.
#include "scrub_common.hpp"

namespace rmq {
namespace {

__device__ __forceinline__ u32 uni(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ u64 uni(u64 v) { return ((u64)uni((u32)(v >> 32)) << 32) | uni((u32)v); }

// The bytes [pos, end) at base, each address masked with `mask`, as ONE §10 segment from `expect`:
// header offsets in sequence, extent inside the span, CRC32C, zero padding, landing exactly on
// `end` with expect == eoff (the rule set of the verified fetch). The whole wave calls it with the
// same arguments and walks record by record; a record over kBigScrub pieces is folded by the wave
// (the 1 KB Horner shift), a smaller one runs the register through its pieces.
__device__ __forceinline__ bool span_walk(const uint8_t* base, u64 mask, u64 pos, u64 end, u64 expect, u64 eoff,
                                          const CrcConsts* crc, const u32 (*t8)[256]) {
  while (pos < end) {
    const uint4 h = load_payload16(base + (pos & mask));
    const u64 off = ((u64)uni(h.y) << 32) | uni(h.x);
    const u32 L = uni(h.z), want = uni(h.w);
    const u32 m = (L >> 4) + ((L & 15u) ? 1u : 0u);
    const u64 avail = ((end - pos) >> 4) - 1ull;  // pieces of the span after this header
    if (off != expect || (u64)m > avail) return false;
    const u64 pay = pos + 16ull;
    u32 acc = 0xFFFFFFFFu;
    bool padz = true;
    if (m > kBigScrub) {
      acc = wave_crc_pieces(crc, t8, m, [&](u32 jp) { return load_payload16(base + ((pay + 16ull * jp) & mask)); });
      padz = pad_zero16(load_payload16(base + ((pos + 16ull * m) & mask)), L);
    } else {
      for (u32 c = 0; c < m; ++c) {
        const uint4 v = load_payload16(base + ((pay + 16ull * c) & mask));
        acc = crc_step8(t8, crc_step8(t8, acc, v.x, v.y), v.z, v.w);
        if (c + 1u == m) padz = pad_zero16(v, L);
      }
    }
    if (uni(crc_of_padded(crc, acc, L, m)) != want || !uni((u32)padz)) return false;
    pos += 16ull * (1ull + m);
    ++expect;
  }
  return expect == eoff;
}

// wave -> (source or destination rank q, entry k of its list)
__device__ __forceinline__ u32 rank_of_wave(const uint32_t* w0, u32 world, u32 w) {
  u32 q = 0;
  while (q + 1u < world && w0[q + 1u] <= w) ++q;
  return q;
}

// The donor's local pidx of a placement key, or ~0.
__device__ __forceinline__ u32 resolve_key(const RemoteKey* keys, u32 n, u32 P, u64 key) {
  u32 a = 0, b = n;
  while (a < b) {
    const u32 mid = a + ((b - a) >> 1);
    if (keys[mid].key < key) a = mid + 1u; else b = mid;
  }
  if (a >= n || keys[a].key != key || keys[a].pidx >= P) return ~0u;
  return keys[a].pidx;
}

__device__ __forceinline__ u64 wave_sum(u64 v) { return bcast_u64(wave_incl_scan(v), 63u); }

}  // namespace

// The verify grid again: waves stride over blocks of 64 tasks, a lane per task.
__global__ __launch_bounds__(kST) void remote_request_kernel(RemoteReqArgs Q) {
  const ScrubArgs& A = Q.r.s;
  const DevState& st = A.st;
  const u32 lane = threadIdx.x & 63u;
  const u64 T = A.tbase[A.n];
  const u64 stride = 64ull * gridDim.x * kSW;
  unsigned long long* ctr = reinterpret_cast<unsigned long long*>(Q.ctr);
  for (u64 t0 = 64ull * (u32)__builtin_amdgcn_readfirstlane(blockIdx.x * kSW + (threadIdx.x >> 6)); t0 < T; t0 += stride) {
    const u64 t = t0 + lane;
    if (t >= T) continue;
    const bool look = Q.round == 0u ? Q.r.verdict[t] != kVerdictPass : Q.want[t] != 0;
    if (!look) {
      if (Q.round == 0u) Q.want[t] = 0;
      continue;
    }
    const ScrubTask k = scrub_task(A, t);
    if (Q.round == 0u) {
      // no passing local slot, as repair_copy_kernel finds it: such a pair was left unrepaired
      bool have = false;
      const u64 vb = A.tbase[k.i] + k.s;
      u32 mk = k.mask;
      for (u64 j = 0; mk && !have; ++j, mk &= mk - 1u) have = j != k.ri && Q.r.verdict[vb + j * k.nseg] == kVerdictPass;
      Q.want[t] = have ? 0 : 1;
      if (have) continue;
    }
    // a segment with bounds whose records are all committed here (FORMAT.md §10: only the committed
    // prefix is identical on every replica)
    if (k.kind || k.pos >= k.end || k.eoff > st.commit[A.first + k.i]) continue;
    const u32 d = Q.cand[(u64)k.i * Q.ncand + Q.round];
    if (d >= Q.world) continue;  // (~0: no candidate left)
    atomicAdd(ctr + 2u * Q.world, 1ull);
    const u64 len = k.end - k.pos;
    const u64 before = atomicAdd(ctr + Q.world + d, (unsigned long long)len);
    if (before + len > Q.peer_bytes) {  // over the destination's budget: a later round or call
      atomicAdd(ctr + Q.world + d, (unsigned long long)(0ull - len));
      continue;
    }
    const u64 idx = atomicAdd(ctr + d, 1ull);
    if (idx >= Q.max_reqs) continue;
    u64* rq = reinterpret_cast<u64*>(Q.lists + (u64)d * Q.list_cap + kRemoteHdr + (u64)kRemoteReq * idx);
    rq[0] = Q.pkey[A.first + k.i];
    rq[1] = k.pos;
    rq[2] = k.end;
    rq[3] = k.expect;
    rq[4] = k.eoff;
    rq[5] = t;
  }
}

// One wave per request received: the checks and the in-place walk. sv[w] = span bytes | slot << 48
// | status << 60; the bytes of the accepted spans go into the source's chunk sums and totals.
__global__ __launch_bounds__(kST) void remote_serve_check_kernel(RemoteServeArgs S) {
  __shared__ __attribute__((aligned(16))) u32 tabs[16 * 256];  // table[8] then zshift[2][4]
  __shared__ __attribute__((aligned(16))) u32 nibs[512];
  crc_tables_lds<kST>(S.crc, tabs, nibs);
  __syncthreads();
  const u32(*t8)[256] = reinterpret_cast<const u32(*)[256]>(tabs);
  const DevState& st = S.st;
  const u32 w = uni(blockIdx.x * kSW + (threadIdx.x >> 6));
  if (w >= S.w0[S.world]) return;
  const u32 q = rank_of_wave(S.w0, S.world, w);
  const u32 k = w - S.w0[q];
  const uint8_t* list = S.in + S.in_off[q];
  const u32 dry = uni(reinterpret_cast<const u32*>(list)[3]) & kRemoteDry;
  const u64* rq = reinterpret_cast<const u64*>(list + kRemoteHdr + (u64)kRemoteReq * k);
  const u64 key = uni(rq[0]), pos = uni(rq[1]), end = uni(rq[2]), expect = uni(rq[3]), eoff = uni(rq[4]);
  u32 status = kRemoteUnknown, slot = 0;
  u64 len = 0;
  const u32 p = resolve_key(S.keys, S.nkeys, st.P, key);
  if (p != ~0u) {
    const ScrubPart g = scrub_part(st, p);
    if (g.mask) {
      status = kRemoteOutside;
      const u64 top = g.eo < st.commit[p] ? g.eo : st.commit[p];
      if (g.sane && ((pos | end) & 15ull) == 0ull && g.sp <= pos && pos < end && end <= g.ep && end - pos <= g.rg.seg &&
          g.so <= expect && expect <= eoff && eoff <= top) {
        status = kRemoteBadWalk;
        // the lowest local slot on which the span passes
        for (u32 mk = g.mask; mk && status != kRemoteServed; mk &= mk - 1u) {
          const u32 r = (u32)__builtin_ctz(mk);
          const uint8_t* ring = st.logs + (u64)r * st.rstride + g.rg.base;
          if (span_walk(ring, g.rg.seg - 1ull, pos, end, expect, eoff, S.crc, t8)) {
            status = kRemoteServed;
            slot = r;
            len = end - pos;
          }
        }
      }
    }
  }
  if ((threadIdx.x & 63u) == 0u) {
    S.sv[w] = len | ((u64)slot << 48) | ((u64)status << 60);
    if (status == kRemoteServed) {
      unsigned long long* tot = reinterpret_cast<unsigned long long*>(S.tot + 3ull * q);
      atomicAdd(tot, 1ull);
      atomicAdd(tot + 1, (unsigned long long)len);
      if (!dry) {
        atomicAdd(tot + 2, (unsigned long long)len);
        atomicAdd(reinterpret_cast<unsigned long long*>(S.csum + (u64)q * kRemoteChunks + k / kRemoteChunk),
                  (unsigned long long)len);
      }
    }
  }
}

// One wave per request again: its directory entry, and the copy of a passing span behind the
// spans accepted before it in the source's list (wave 0 of a source writes the header).
__global__ __launch_bounds__(kST) void remote_serve_copy_kernel(RemoteServeArgs S) {
  const DevState& st = S.st;
  const u32 lane = threadIdx.x & 63u;
  const u32 w = uni(blockIdx.x * kSW + (threadIdx.x >> 6));
  if (w >= S.w0[S.world]) return;
  const u32 q = rank_of_wave(S.w0, S.world, w);
  const u32 k = w - S.w0[q], n = S.w0[q + 1u] - S.w0[q];
  const uint8_t* list = S.in + S.in_off[q];
  const u32 dry = uni(reinterpret_cast<const u32*>(list)[3]) & kRemoteDry;
  const u64* rq = reinterpret_cast<const u64*>(list + kRemoteHdr + (u64)kRemoteReq * k);
  const u64 v = uni(S.sv[w]);
  const u32 status = (u32)(v >> 60), slot = (u32)(v >> 48) & 0xFFu;
  const u64 len = v & ((1ull << 48) - 1ull);
  // data bytes before this span: the chunks before its own, then the spans before it in its chunk
  u64 mine = 0;
  if (!dry) {
    const u32 c = k / kRemoteChunk;
    for (u32 j = lane; j < c; j += 64u) mine += S.csum[(u64)q * kRemoteChunks + j];
    for (u32 j = lane; j < k - c * kRemoteChunk; j += 64u) {
      const u64 o = S.sv[S.w0[q] + c * kRemoteChunk + j];
      mine += (o >> 60) == kRemoteServed ? o & ((1ull << 48) - 1ull) : 0ull;
    }
  }
  const u64 start = wave_sum(mine);
  uint8_t* out = S.out + S.out_off[q];
  if (lane == 0u) {
    u64* d = reinterpret_cast<u64*>(out + kRemoteHdr + (u64)kRemoteDir * k);
    d[0] = uni(rq[5]);  // the cookie, echoed
    d[1] = (u64)status | ((dry ? 0ull : start >> 4) << 32);
    if (k == 0u) {
      u64* h = reinterpret_cast<u64*>(out);
      h[0] = (u64)kRemoteMagic | ((u64)n << 32);
      h[1] = S.tot[3ull * q + 2];
    }
  }
  if (status != kRemoteServed || dry) return;
  const u32 p = resolve_key(S.keys, S.nkeys, st.P, uni(rq[0]));
  if (p == ~0u) return;  // (served: the check kernel resolved it)
  const RingRef rg = ring_ref(st, p);
  const uint8_t* ring = st.logs + (u64)slot * st.rstride + rg.base;
  const u64 pos = uni(rq[1]), m = rg.seg - 1ull;
  uint8_t* dst = out + kRemoteHdr + (u64)kRemoteDir * n + start;
  for (u64 o = 16ull * lane; o < len; o += 1024ull)
    *reinterpret_cast<uint4*>(dst + o) = load_payload16(ring + ((pos + o) & m));
}

// One wave per directory entry received: structure, the walk of the span in the inbox against the
// rank's own task, then the copy into the failing slot's ring.
__global__ __launch_bounds__(kST) void remote_install_kernel(RemoteInstallArgs I) {
  __shared__ __attribute__((aligned(16))) u32 tabs[16 * 256];
  __shared__ __attribute__((aligned(16))) u32 nibs[512];
  const ScrubArgs& A = I.r.s;
  crc_tables_lds<kST>(A.crc, tabs, nibs);
  __syncthreads();
  const u32(*t8)[256] = reinterpret_cast<const u32(*)[256]>(tabs);
  const u32 lane = threadIdx.x & 63u;
  const u32 w = uni(blockIdx.x * kSW + (threadIdx.x >> 6));
  if (w >= I.w0[I.world]) return;
  const u32 q = rank_of_wave(I.w0, I.world, w);
  const u32 k = w - I.w0[q], n = I.w0[q + 1u] - I.w0[q];
  const uint8_t* reg = I.in + I.in_off[q];
  const u64 bytes = I.in_bytes[q], dirend = kRemoteHdr + (u64)kRemoteDir * n;
  if (bytes < dirend) return;
  const u64 h0 = uni(reinterpret_cast<const u64*>(reg)[0]), data = uni(reinterpret_cast<const u64*>(reg)[1]);
  if (h0 != ((u64)kRemoteMagic | ((u64)n << 32)) || data != bytes - dirend) return;
  const u64* d = reinterpret_cast<const u64*>(reg + kRemoteHdr + (u64)kRemoteDir * k);
  const u64 t = uni(reinterpret_cast<const u64*>(I.lists + (u64)q * I.list_cap + kRemoteHdr + (u64)kRemoteReq * k)[5]);
  const u64 d1 = uni(d[1]);
  if (uni(d[0]) != t || (u32)d1 != kRemoteServed) return;  // not the entry of this request, or refused
  if (t >= A.tbase[A.n] || !I.want[t]) return;
  const ScrubTask s = scrub_task(A, t);
  if (s.kind || s.pos >= s.end) return;
  const u64 len = s.end - s.pos;
  if (I.r.write) {
    // the directory tiles the data section in request order
    const u64 start = (d1 >> 32) << 4;
    const u64 next = k + 1u < n ? (uni(d[3]) >> 32) << 4 : data;
    if ((k == 0u && start) || start + len > data || start + len != next) return;
    const uint8_t* span = reg + dirend + start;
    if (!span_walk(span, ~0ull, 0, len, s.expect, s.eoff, A.crc, t8)) return;  // writes nothing
    uint8_t* ring = const_cast<uint8_t*>(s.ring);
    for (u64 o = 16ull * lane; o < len; o += 1024ull) store_log16(ring + ((s.pos + o) & s.rmask), load_payload16(span + o));
  } else if (data) {
    return;  // a dry response carries no data
  }
  if (lane == 0u) {
    I.want[t] = 0;
    I.r.verdict[t] = kVerdictPass;
    unsigned long long* f = reinterpret_cast<unsigned long long*>(I.fetched + 2ull * s.i);
    atomicAdd(f, 1ull);
    atomicAdd(f + 1, (unsigned long long)len);
  }
}

void launch_remote_request(const RemoteReqArgs& a, uint32_t wgs, hipStream_t s) {
  hipLaunchKernelGGL(remote_request_kernel, dim3(wgs), dim3(kST), 0, s, a);
}

void launch_remote_serve_check(const RemoteServeArgs& a, hipStream_t s) {
  const uint32_t waves = a.w0[a.world];
  if (waves) hipLaunchKernelGGL(remote_serve_check_kernel, dim3((waves + kSW - 1) / kSW), dim3(kST), 0, s, a);
}

void launch_remote_serve_copy(const RemoteServeArgs& a, hipStream_t s) {
  const uint32_t waves = a.w0[a.world];
  if (waves) hipLaunchKernelGGL(remote_serve_copy_kernel, dim3((waves + kSW - 1) / kSW), dim3(kST), 0, s, a);
}

void launch_remote_install(const RemoteInstallArgs& a, hipStream_t s) {
  const uint32_t waves = a.w0[a.world];
  if (waves) hipLaunchKernelGGL(remote_install_kernel, dim3((waves + kSW - 1) / kSW), dim3(kST), 0, s, a);
}

}  // namespace rmq
