// repair.hip — rewriting damaged replica logs from a clean local replica (rmq_repair, FORMAT.md
// §10 "Repair"), gfx950.
//
// The first pass is the scrub's plan and verify walk (scrub_common.hpp) with one verdict byte
// stored per task. The repair kernel then takes the same tasks, 64 to a wave: a lane decodes its
// (partition, local slot, segment), and for a failing one looks up the verdicts of the same
// segment on the partition's other local slots. The wave then copies each failing segment that
// has a passing slot from the lowest such slot, 64 lanes x 16 bytes a step.
//
// Bounds: the copy covers [pos, end) of scrub_task, which come from the index entries and the
// partition state after the containment checks (inside [log_start_pos, log_end_pos) of a log no
// longer than its ring, 16-byte aligned) and never from a record's length word; a segment that
// failed them has pos = end = 0 and fails on every slot alike, so it has neither bounds nor a
// donor. Both addresses of every piece are masked with S_p - 1 of the partition's ring. A verdict
// index is tbase[i] + k * nseg + s with k < popc(mask) and s < nseg, inside the partition's task
// range. Targets are failing pairs and donors are passing pairs of one first pass, so no byte is
// both read and written.
#include "scrub_common.hpp"

namespace rmq {

__global__ __launch_bounds__(kST, 4) void repair_verify_kernel(ScrubArgs A, uint8_t* verdict) {
  __shared__ __attribute__((aligned(16))) u32 tabs[16 * 256];  // table[8] then zshift[2][4]
  __shared__ __attribute__((aligned(16))) u32 nibs[512];
  scrub_verify_body<true>(A, verdict, tabs, nibs);
}

// The verify grid again: waves stride over blocks of 64 tasks. counts: [n][3] {segments repaired,
// their bytes, segments left unrepaired}. write == 0 (dry run): count only.
__global__ __launch_bounds__(kST) void repair_copy_kernel(RepairArgs R) {
  const ScrubArgs& A = R.s;
  const DevState& st = A.st;
  const u32 lane = threadIdx.x & 63u;
  const u64 T = A.tbase[A.n];
  const u64 stride = 64ull * gridDim.x * kSW;
  for (u64 t0 = 64ull * (u32)__builtin_amdgcn_readfirstlane(blockIdx.x * kSW + (threadIdx.x >> 6)); t0 < T; t0 += stride) {
    const u64 t = t0 + lane;
    bool fail = false, have = false;
    u32 i = 0;
    u64 pos = 0, end = 0, rmask = 0;
    const uint8_t* ring = st.logs;
    const uint8_t* donor = st.logs;
    if (t < T && R.verdict[t] != kVerdictPass) {
      fail = true;
      const ScrubTask k = scrub_task(A, t);
      i = k.i, pos = k.pos, end = k.end, rmask = k.rmask, ring = k.ring;
      // the same segment on the partition's other local slots, lowest slot first
      const u64 vb = A.tbase[i] + k.s;
      u32 mk = k.mask;
      for (u64 j = 0; mk && !have; ++j, mk &= mk - 1u) {
        if (j == k.ri || R.verdict[vb + j * k.nseg] != kVerdictPass) continue;
        have = true;
        donor = ring - (u64)k.r * st.rstride + (u64)(u32)__builtin_ctz(mk) * st.rstride;
      }
      unsigned long long* cnt = reinterpret_cast<unsigned long long*>(R.counts + 3ull * i);
      if (have) {
        atomicAdd(cnt, 1ull);
        atomicAdd(cnt + 1, (unsigned long long)(end - pos));
      } else {
        atomicAdd(cnt + 2, 1ull);
      }
    }
    // each repairable segment by the whole wave
    for (u64 bm = R.write ? __ballot(fail && have) : 0ull; bm; bm &= bm - 1ull) {
      const u32 sl = (u32)__builtin_ctzll(bm);
      uint8_t* dst = reinterpret_cast<uint8_t*>(bcast_u64(reinterpret_cast<u64>(ring), sl));
      const uint8_t* src = reinterpret_cast<const uint8_t*>(bcast_u64(reinterpret_cast<u64>(donor), sl));
      const u64 e = bcast_u64(end, sl), m = bcast_u64(rmask, sl);
      for (u64 o = bcast_u64(pos, sl) + 16ull * lane; o < e; o += 1024ull) store_log16(dst + (o & m), load_payload16(src + (o & m)));
    }
  }
}

void launch_repair_scan(const RepairArgs& a, uint32_t wgs, hipStream_t s) {
  launch_scrub_plan(a.s, s);
  hipLaunchKernelGGL(repair_verify_kernel, dim3(wgs), dim3(kST), 0, s, a.s, a.verdict);
}

void launch_repair_copy(const RepairArgs& a, uint32_t wgs, hipStream_t s) {
  hipLaunchKernelGGL(repair_copy_kernel, dim3(wgs), dim3(kST), 0, s, a);
}

}  // namespace rmq
