// lag.cpp — rmq_lag of the C-ABI (FORMAT.md §7 "Lag"): per (partition, reader) row the backlog in
// records and bytes and the partition's retention headroom.
//
// The call is ordered as a fetch is: its one kernel goes to the pipeline stream under the engine lock,
// after every launch issued before it and before the ones issued after it, and the host waits for
// that kernel alone. It takes no fetch slot, flushes and drains nothing, and writes nothing of the
// engine. Its steps are the functions below, in their order: check, scan flags, stage, launch, wait,
// copy back.
#include "engine_internal.hpp"

using namespace rmq;

namespace rmq {

namespace {

struct LagCall {
  const rmq_fetch_req* reqs;
  const uint64_t* offsets;
  uint32_t n, mem;
  rmq_lag_res* res;
};

// Step 1, the argument checks: nothing of the engine is read, nothing runs.
int lag_check(const rmq_engine* e, const LagCall& c) {
  if (!e) return RMQ_EINVAL;
  if (c.mem != RMQ_MEM_HOST && c.mem != RMQ_MEM_DEVICE) return RMQ_EINVAL;  // (any RMQ_FETCH_* bit included)
  if (c.n && (!c.reqs || !c.res)) return RMQ_EINVAL;
  if (c.mem == RMQ_MEM_DEVICE &&
      (((reinterpret_cast<uintptr_t>(c.reqs) | reinterpret_cast<uintptr_t>(c.res)) & 15u) ||
       (reinterpret_cast<uintptr_t>(c.offsets) & 7u)))
    return RMQ_EINVAL;
  return RMQ_OK;
}

// Step 2, host rows: known flag bits only (device rows are never read here: only their replica bit
// is looked at, by the kernel).
int lag_scan_flags(const LagCall& c) {
  if (c.mem != RMQ_MEM_HOST) return RMQ_OK;
  uint32_t fl = 0;
  for (uint32_t r = 0; r < c.n; ++r) fl |= c.reqs[r].flags;
  return fl & ~(RMQ_FETCH_COMMIT | RMQ_FETCH_REPLICA | RMQ_FETCH_VERIFY) ? RMQ_EINVAL : RMQ_OK;
}

// Step 3: host rows and offsets into the call's page-locked scratch (grown on demand, never shrunk),
// which the kernel reads and writes in place; device rows are used where they are.
int lag_stage(rmq_engine* e, const LagCall& c, LagArgs& a) {
  rmq_engine::Lag& l = e->lag;
  if (!l.ev) HIP_TRY(hipEventCreateWithFlags(&l.ev, hipEventDisableTiming));
  a.req = reinterpret_cast<const uint32_t*>(c.reqs);
  a.at = c.offsets;
  a.res = reinterpret_cast<uint64_t*>(c.res);
  a.n = c.n;
  if (c.mem != RMQ_MEM_HOST) return RMQ_OK;
  if (c.n > l.cap) {
    lag_free(e);
    const uint32_t cap = std::max<uint32_t>(c.n, 1024);
    HIP_TRY(hipHostMalloc((void**)&l.h_req, (size_t)cap * sizeof(rmq_fetch_req), 0));
    HIP_TRY(hipHostMalloc((void**)&l.h_at, (size_t)cap * 8, 0));
    HIP_TRY(hipHostMalloc((void**)&l.h_res, (size_t)cap * sizeof(rmq_lag_res), 0));
    l.cap = cap;
  }
  std::memcpy(l.h_req, c.reqs, (size_t)c.n * sizeof(rmq_fetch_req));
  if (c.offsets) std::memcpy(l.h_at, c.offsets, (size_t)c.n * 8);
  a.req = reinterpret_cast<const uint32_t*>(l.h_req);
  a.at = c.offsets ? l.h_at : nullptr;
  a.res = reinterpret_cast<uint64_t*>(l.h_res);
  return RMQ_OK;
}

// Step 4, under the engine lock: the kernel on the pipeline stream, behind the fetches held back and
// the retention of every batch applied so far (the log starts it reads), an event after it. Profile
// region 10: an event before the kernel to one after it.
int lag_launch(rmq_engine* e, LagArgs& a) {
  EngineLock g(e);
  int rc = late_retention(e);
  if (rc) return rc;
  a.st = e->st;
  hipEvent_t t1 = nullptr;
  if (e->profile) {
    const hipEvent_t t0 = pool_event(e);
    t1 = pool_event(e);
    e->prof[10].push_back({t0, t1});
    HIP_TRY(hipEventRecord(t0, e->main_s));
  }
  launch_lag(a, e->main_s);
  HIP_TRY(hipGetLastError());
  if (t1) HIP_TRY(hipEventRecord(t1, e->main_s));
  HIP_TRY(hipEventRecord(e->lag.ev, e->main_s));
  return RMQ_OK;
}

}  // namespace

void lag_free(rmq_engine* e) {
  rmq_engine::Lag& l = e->lag;
  for (void** p : {(void**)&l.h_req, (void**)&l.h_at, (void**)&l.h_res}) {
    if (*p) hipHostFree(*p);
    *p = nullptr;
  }
  l.cap = 0;
}

}  // namespace rmq

extern "C" {

int rmq_lag(rmq_engine* e, const rmq_fetch_req* reqs, const uint64_t* offsets, uint32_t n, uint32_t mem,
            rmq_lag_res* res) {
  static_assert(sizeof(rmq_lag_res) == 64 && offsetof(rmq_lag_res, status) == 56, "result rows are eight words");
  const LagCall c{reqs, offsets, n, mem, res};
  int rc = lag_check(e, c);
  if (!rc) rc = lag_scan_flags(c);
  if (rc || !n) return rc;
  std::lock_guard<std::mutex> lg(e->lag_mu);  // the scratch and the event, until the rows are copied back
  HIP_TRY(hipSetDevice(e->device));
  LagArgs a{};
  rc = lag_stage(e, c, a);
  if (!rc) rc = lag_launch(e, a);
  if (!rc) rc = event_wait(e->lag.ev);
  if (rc) return rc;
  if (mem == RMQ_MEM_HOST) std::memcpy(res, e->lag.h_res, (size_t)n * sizeof(rmq_lag_res));
  return RMQ_OK;
}

}  // extern "C"
