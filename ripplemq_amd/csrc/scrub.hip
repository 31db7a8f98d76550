// scrub.hip — on-device audit of the retained logs (rmq_scrub, FORMAT.md §10), gfx950.
//
// A ring holds no record table, but the sparse index (FORMAT.md §5) names a record start at or
// after every multiple of the interval, so the live entries tile a partition's retained log into
// segments of about one interval each. A task is (partition, local replica slot, segment): the plan
// kernel counts them per partition and scans the counts, the verify kernel gives 64 consecutive
// tasks to a wave, one lane per segment. A lane walks its segment's headers in order and runs
// each record's CRC32C register through its 16-byte pieces from the LDS slicing tables, as the
// follower's verify_task_lane does (replicate.hip); records over kBigScrub pieces are taken by the
// whole wave, one at a time, with the 1 KB Horner shift. A hot partition's log is thousands of
// segments, so it spreads over as many lanes as it has intervals.
//
// The segments, the task decoding, its bounds and the verify walk live in scrub_common.hpp, which
// the repair (repair.hip) shares.
#include "scrub_common.hpp"

namespace rmq {
namespace {

constexpr u32 kPlanT = 1024;    // the plan's single workgroup: a thread per partition, chunk after chunk

}  // namespace

// Task counts of partitions [first, first + n) and their exclusive scan; the result rows start
// clean. One workgroup: a thread per partition, kPlanT partitions at a time.
__global__ __launch_bounds__(kPlanT) void scrub_plan_kernel(ScrubArgs A) {
  __shared__ u64 wsum[kPlanT / 64];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  u64 carry = 0;
  for (u32 c0 = 0; c0 < A.n; c0 += kPlanT) {  // (uniform)
    const u32 i = c0 + threadIdx.x;
    u64 cnt = 0;
    if (i < A.n) {
      const ScrubPart q = scrub_part(A.st, A.first + i);
      const u32 nloc = (u32)__popc(q.mask);
      cnt = nloc * q.nseg;
      u64* row = A.rows + 4ull * i;
      row[0] = kScrubClean;
      row[1] = 0;
      row[2] = 0;
      row[3] = nloc;
    }
    const u64 incl = wave_incl_scan(cnt);
    if (lane == 63u) wsum[wave] = incl;
    __syncthreads();
    u64 before = 0, total = 0;
#pragma unroll
    for (u32 w = 0; w < kPlanT / 64; ++w) {
      const u64 v = wsum[w];
      before += w < wave ? v : 0ull;
      total += v;
    }
    if (i < A.n) A.tbase[i] = carry + before + incl - cnt;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) A.tbase[A.n] = carry;
}

// A grid of a few workgroups per CU: each builds the CRC tables in LDS once and its waves take
// blocks of 64 tasks w, w + waves, ...
__global__ __launch_bounds__(kST, 4) void scrub_verify_kernel(ScrubArgs A) {
  __shared__ __attribute__((aligned(16))) u32 tabs[16 * 256];  // table[8] then zshift[2][4]
  __shared__ __attribute__((aligned(16))) u32 nibs[512];
  scrub_verify_body<false>(A, nullptr, tabs, nibs);
}

void launch_scrub_plan(const ScrubArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(scrub_plan_kernel, dim3(1), dim3(kPlanT), 0, s, a);
}

void launch_scrub(const ScrubArgs& a, uint32_t verify_wgs, hipStream_t s) {
  launch_scrub_plan(a, s);
  hipLaunchKernelGGL(scrub_verify_kernel, dim3(verify_wgs), dim3(kST), 0, s, a);
}

}  // namespace rmq
