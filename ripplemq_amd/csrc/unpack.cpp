// unpack.cpp — rmq_unpack of the C-ABI (FORMAT.md §7 "Record columns"): the answer of a table fetch
// as per-record columns and a payload area (view, packed or strided).
//
// The call is ordered as a fetch is: its kernels go to the pipeline stream under the engine lock,
// after every launch issued before it and before the ones issued after it, and the host waits for
// its own kernels alone. It takes no fetch slot, flushes and drains nothing, and writes nothing of
// the engine. Its steps are the functions below, in their order: check, stage, launch, wait, answer.
#include "engine_internal.hpp"

using namespace rmq;

namespace rmq {

namespace {

template <typename T>
bool misaligned(const T* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) & (a - 1u); }

// Step 1, the argument checks: nothing of the engine is read, nothing runs.
int unpack_check(const rmq_engine* e, const rmq_unpack_args* a, const rmq_unpack_res* out) {
  if (!e || !a || !out) return RMQ_EINVAL;
  if (a->mem != RMQ_MEM_DEVICE && a->mem != (RMQ_MEM_DEVICE | RMQ_FETCH_DEVICE_ROWS)) return RMQ_EINVAL;
  if (a->flags) return RMQ_EINVAL;
  if (misaligned(a->buf, 16) || misaligned(a->rec_row, 8) || misaligned(a->rec_pos, 8) || misaligned(a->row_tag, 4) ||
      misaligned(a->rec_first, 8) || misaligned(a->offset, 8) || misaligned(a->len, 4) || misaligned(a->payload_off, 8) ||
      misaligned(a->tag, 4))
    return RMQ_EINVAL;
  if ((a->mem & RMQ_FETCH_DEVICE_ROWS) && misaligned(a->rows, 16)) return RMQ_EINVAL;
  // the mode: view takes no payload area; a stride needs one
  if (!a->payload && (a->stride || a->payload_cap)) return RMQ_EINVAL;
  if (!a->n) return RMQ_OK;
  if (!a->rows || !a->rec_row || !a->rec_first) return RMQ_EINVAL;
  if ((a->rec_words && !a->rec_pos) || (a->buf_bytes && !a->buf)) return RMQ_EINVAL;
  if (a->rec_cap && (!a->len || !a->payload_off)) return RMQ_EINVAL;
  return RMQ_OK;
}

// Step 2: the scratch of the call (grown on demand, never shrunk), and host rows through the
// page-locked staging into their device copy, on the pipeline stream in step 3.
int unpack_stage(rmq_engine* e, const rmq_unpack_args& c, UnpackArgs& a) {
  rmq_engine::Unpack& u = e->unpack;
  if (!u.ev) HIP_TRY(hipEventCreateWithFlags(&u.ev, hipEventDisableTiming));
  if (!u.h_ctl) {
    HIP_TRY(hipHostMalloc((void**)&u.h_ctl, kUnpackCtlWords * 8, 0));
    HIP_TRY(hipMalloc((void**)&u.d_ctl, kUnpackCtlWords * 8));
  }
  if (c.n > u.row_cap) {
    if (u.h_rows) hipHostFree(u.h_rows);
    if (u.d_rows) hipFree(u.d_rows);
    if (u.d_rsum) hipFree(u.d_rsum);
    u.h_rows = nullptr, u.d_rows = nullptr, u.d_rsum = nullptr, u.row_cap = 0;
    const uint32_t cap = std::max<uint32_t>(c.n, 1024);
    if (hipHostMalloc((void**)&u.h_rows, (size_t)cap * sizeof(rmq_fetch_res), 0) != hipSuccess ||
        hipMalloc((void**)&u.d_rows, (size_t)cap * sizeof(rmq_fetch_res)) != hipSuccess ||
        hipMalloc((void**)&u.d_rsum, ((size_t)cap / kFetchChunk + 1) * 8) != hipSuccess) {
      (void)hipGetLastError();
      return RMQ_ENOMEM;
    }
    u.row_cap = cap;
  }
  int rc = restore_grow(&u.d_lsum, &u.lsum_cap, std::max<uint64_t>(c.rec_words / kUnpackChunk + 1, 1024));
  if (rc) return rc;
  a.buf = c.buf, a.buf_bytes = c.buf_bytes;
  a.rec_row = c.rec_row, a.rec_pos = c.rec_pos, a.rec_words = c.rec_words, a.row_tag = c.row_tag;
  a.rec_first = c.rec_first, a.offset = c.offset, a.len = c.len, a.payload_off = c.payload_off, a.tag = c.tag;
  a.rec_cap = c.rec_cap, a.payload = c.payload, a.payload_cap = c.payload_cap;
  a.rsum = u.d_rsum, a.lsum = u.d_lsum, a.ctl = u.d_ctl;
  a.n = c.n, a.stride = c.stride;
  a.mode = !c.payload ? kUnpackView : c.stride ? kUnpackStrided : kUnpackPacked;
  if (c.mem & RMQ_FETCH_DEVICE_ROWS) {
    a.rows = reinterpret_cast<const uint64_t*>(c.rows);
  } else {
    std::memcpy(u.h_rows, c.rows, (size_t)c.n * sizeof(rmq_fetch_res));
    a.rows = u.d_rows;
  }
  return RMQ_OK;
}

// Step 3, under the engine lock: everything on the pipeline stream, behind the fetches held back:
// the control words zeroed, host rows to the device, the kernels, the control words back, an event.
// Profile region 11: an event before the first kernel to one after the last.
int unpack_launch(rmq_engine* e, const rmq_unpack_args& c, const UnpackArgs& a) {
  EngineLock g(e);
  rmq_engine::Unpack& u = e->unpack;
  if (!c.n) {  // no row: rec_first[0] = 0 is the whole answer
    HIP_TRY(hipMemsetAsync(c.rec_first, 0, 8, e->main_s));
    HIP_TRY(hipEventRecord(u.ev, e->main_s));
    return RMQ_OK;
  }
  HIP_TRY(hipMemsetAsync(u.d_ctl, 0, kUnpackCtlWords * 8, e->main_s));
  if (!(c.mem & RMQ_FETCH_DEVICE_ROWS))
    HIP_TRY(hipMemcpyAsync(u.d_rows, u.h_rows, (size_t)c.n * sizeof(rmq_fetch_res), hipMemcpyHostToDevice, e->main_s));
  hipEvent_t t1 = nullptr;
  if (e->profile) {
    const hipEvent_t t0 = pool_event(e);
    t1 = pool_event(e);
    e->prof[11].push_back({t0, t1});
    HIP_TRY(hipEventRecord(t0, e->main_s));
  }
  launch_unpack(a, audit_wgs(e), e->main_s);
  HIP_TRY(hipGetLastError());
  if (t1) HIP_TRY(hipEventRecord(t1, e->main_s));
  HIP_TRY(hipMemcpyAsync(u.h_ctl, u.d_ctl, kUnpackCtlWords * 8, hipMemcpyDeviceToHost, e->main_s));
  HIP_TRY(hipEventRecord(u.ev, e->main_s));
  return RMQ_OK;
}

// Step 5: the answer from the control words.
int unpack_answer(const rmq_unpack_args& c, const uint64_t* ctl, rmq_unpack_res* out) {
  if (ctl[kUnpackBad]) {
    out->bad_row = c.n - ctl[kUnpackBad];
    out->status = RMQ_EINVAL;
    return RMQ_EINVAL;
  }
  out->records = ctl[kUnpackRecords];
  out->payload_bytes = ctl[kUnpackBytes];
  out->mismatched = ctl[kUnpackMismatch];
  out->truncated = ctl[kUnpackTrunc];
  out->status = ctl[kUnpackStop] ? RMQ_ENOSPC : RMQ_OK;
  return out->status;
}

}  // namespace

void unpack_free(rmq_engine* e) {
  rmq_engine::Unpack& u = e->unpack;
  if (u.h_rows) hipHostFree(u.h_rows);
  if (u.h_ctl) hipHostFree(u.h_ctl);
  for (uint64_t* p : {u.d_rows, u.d_rsum, u.d_lsum, u.d_ctl})
    if (p) hipFree(p);
  if (u.ev) hipEventDestroy(u.ev);
  u = rmq_engine::Unpack{};
}

}  // namespace rmq

extern "C" {

int rmq_unpack(rmq_engine* e, const rmq_unpack_args* a, rmq_unpack_res* out) {
  static_assert(sizeof(rmq_unpack_res) == 48 && offsetof(rmq_unpack_res, status) == 40, "the result is six words");
  static_assert(sizeof(rmq_unpack_args) == 136 && offsetof(rmq_unpack_args, n) == 120, "the arguments are seventeen words");
  int rc = unpack_check(e, a, out);
  if (rc) return rc;
  *out = rmq_unpack_res{0, 0, 0, 0, RMQ_OFFSET_NONE, RMQ_OK, 0};
  if (!a->n && !a->rec_first) return RMQ_OK;
  std::lock_guard<std::mutex> lg(e->unpack_mu);  // the scratch and the event, until the answer is read
  HIP_TRY(hipSetDevice(e->device));
  UnpackArgs k{};
  if (a->n) rc = unpack_stage(e, *a, k);
  else if (!e->unpack.ev) HIP_TRY(hipEventCreateWithFlags(&e->unpack.ev, hipEventDisableTiming));
  if (!rc) rc = unpack_launch(e, *a, k);
  if (!rc) rc = event_wait(e->unpack.ev);
  if (rc) {
    out->status = rc;
    return rc;
  }
  return a->n ? unpack_answer(*a, e->unpack.h_ctl, out) : RMQ_OK;
}

}  // extern "C"
