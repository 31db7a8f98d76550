// fetch.cpp — the fetch calls of the C-ABI: rmq_fetch, rmq_fetch_bytes, rmq_fetch_at, rmq_fetch_table,
// their _async twins and rmq_fetch_poll (FORMAT.md §7).
//
// A fetch runs in one of the engine's slots (rmq_engine::FetchSlot), serialised by fetch_mu: its
// kernels go to the pipeline stream under the engine lock, ordered after every launch issued before
// it and before the ones issued after it, and the host waits only in rmq_fetch_poll. The ten entry
// points hand one FetchCall to fetch_issue, whose steps are the functions below, in their order.
#include "engine_internal.hpp"

using namespace rmq;

namespace rmq {

namespace {

// Scratch of a fetch slot for n requests and, for a host output, out_cap bytes of device staging.
// Plain hipMalloc (no zeroing, no device synchronisation: a slot first used while the pipeline
// runs must not wait for it; every word a fetch reads is written by it first).
int fetch_alloc(void** p, size_t bytes) {
  *p = nullptr;
  HIP_TRY(hipMalloc(p, std::max<size_t>(bytes, 16)));
  return RMQ_OK;
}

// The scratch of a slot that is sized by its capacity in requests, freed together when the slot grows
// and when the engine goes (the lazily made ones too: their next use makes them again). d_out and
// d_tpos grow on their own (out_alloc, tpos_alloc).
void fetch_slot_drop(rmq_engine::FetchSlot& f) {
  void** dev[] = {(void**)&f.d_req,  (void**)&f.d_res, (void**)&f.d_aux,       (void**)&f.d_cpre, (void**)&f.d_csum,
                  (void**)&f.d_bud,  (void**)&f.d_at,  (void**)&f.d_csum_fill, (void**)&f.d_tsum, (void**)&f.d_trow};
  void** host[] = {(void**)&f.h_req, (void**)&f.h_res, (void**)&f.h_bud, (void**)&f.h_at};
  for (void** p : dev) {
    if (*p) hipFree(*p);
    *p = nullptr;
  }
  for (void** p : host) {
    if (*p) hipHostFree(*p);
    *p = nullptr;
  }
  f.cap = 0;
}

// The slot's staging of a host output or of a host rec_pos, grown (never shrunk) to `need` elements.
int fetch_grow(void** p, uint64_t* have, uint64_t need, size_t elem) {
  if (need <= *have) return RMQ_OK;
  if (*p) hipFree(*p);
  *p = nullptr;
  *have = 0;
  const int rc = fetch_alloc(p, (size_t)need * elem);
  if (!rc) *have = need;
  return rc;
}

int fetch_slot_reserve(rmq_engine::FetchSlot& f, uint32_t n, uint64_t stage, hipStream_t s) {
  if (n > f.cap) {
    fetch_slot_drop(f);
    const uint32_t cap = std::max<uint32_t>(n, 1024);
    int rc = fetch_alloc((void**)&f.d_req, (size_t)cap * 16);
    if (!rc) rc = fetch_alloc((void**)&f.d_res, ((size_t)cap * 4 + 2) * 8);
    if (!rc) rc = fetch_alloc((void**)&f.d_aux, (size_t)cap * 16);
    if (!rc) rc = fetch_alloc((void**)&f.d_cpre, ((size_t)cap + 4) * 4);
    const uint32_t lines = cap / kFetchChunk + 2;
    if (!rc) rc = fetch_alloc((void**)&f.d_csum, 2ull * lines * kCsumStride * 8);
    if (!rc) rc = fetch_alloc((void**)&f.d_bud, (size_t)cap * 4);
    if (rc) return rc;
    // both halves start zeroed (stream-ordered before the slot's first fetch)
    HIP_TRY(hipMemsetAsync(f.d_csum, 0, 2ull * lines * kCsumStride * 8, s));
    f.csum_lines = lines;
    f.csum_par = 0;
    HIP_TRY(hipHostMalloc((void**)&f.h_req, (size_t)cap * 16, 0));
    HIP_TRY(hipHostMalloc((void**)&f.h_res, ((size_t)cap * 4 + 2) * 8, 0));  // res, bytes needed
    HIP_TRY(hipHostMalloc((void**)&f.h_bud, (size_t)cap * 4, 0));
    f.cap = cap;
  }
  return fetch_grow((void**)&f.d_out, &f.out_alloc, stage, 1);
}

// An event of the slot's fetch: RMQ_PENDING while it has not come (wait: block instead).
int fetch_await(hipEvent_t ev, bool wait) {
  if (wait) return event_wait(ev);
  const hipError_t q = hipEventQuery(ev);
  return q == hipErrorNotReady ? RMQ_PENDING : hip_fail(q);
}

// Advance the fetch in slot f (fetch_mu held): RMQ_PENDING while its kernels or host copies run
// (wait: block instead); else its result, with the caller's res (and host output) filled and the
// slot idle again.
int fetch_slot_step(rmq_engine* e, rmq_engine::FetchSlot& f, bool wait, uint64_t* bytes_used) {
  if (f.phase == 1) {
    std::lock_guard<std::mutex> g(e->mu);  // a held-back ticket is launched (with the others held) when polled
    if (f.pending) {
      const int rc = fetch_flush(e);
      if (rc) return rc;
    }
  }
  if (f.phase == 1) {
    const int rc = fetch_await(f.ev, wait);
    if (rc) return rc;
    // the device writes rmq_fetch_res rows (status zero-extended into its reserved word)
    static_assert(sizeof(rmq_fetch_res) == 32, "result rows are four words");
    if (!f.rows_pinned) std::memcpy(f.res, f.h_res, (size_t)f.n * 32);  // (pinned: written in place)
    // some request did not fit iff the bytes needed exceed the output (requests are placed in
    // order: the one holding byte out_cap is cut), so no pass over the rows
    f.rc = __atomic_load_n(f.need, __ATOMIC_ACQUIRE) > f.out_cap ? RMQ_ENOSPC : RMQ_OK;
    // (a table that needs more words than rec_cap: the same code, told apart by rec_row[n] > rec_cap)
    if (f.table && __atomic_load_n(f.tneed, __ATOMIC_ACQUIRE) > f.t_cap) f.rc = RMQ_ENOSPC;
    f.phase = 2;
    if (f.mem == RMQ_MEM_HOST && (f.out_cap || f.t_row)) {
      if (f.t_row) {
        // a host table: rec_row whole, and of rec_pos the words the walk wrote: rows fit while
        // their prefix does (the prefix rises with r), so those are the words before the first row
        // that does not; the others stay untouched in the caller's array, as on the device
        uint64_t words = 0;
        for (uint32_t r = 0; r < f.n; ++r) {
          const uint64_t w = f.res[r].status == RMQ_OK && f.res[r].count ? (uint64_t)f.res[r].count + 1 : 0;
          if (w > f.t_cap - words) break;
          words += w;
        }
        HIP_TRY(hipMemcpyAsync(f.t_row, f.d_trow, ((size_t)f.n + 1) * 8, hipMemcpyDeviceToHost, e->fetch_out_s));
        if (words) HIP_TRY(hipMemcpyAsync(f.t_pos, f.d_tpos, (size_t)words * 8, hipMemcpyDeviceToHost, e->fetch_out_s));
      }
      // copy back the byte runs of the served requests only: the regions of requests that did not
      // fit stay untouched in the caller's buffer, as with a device buffer the gather writes itself
      uint64_t lo = 0, hi = 0;
      for (uint32_t r = 0; f.out_cap && r <= f.n; ++r) {
        const bool served = r < f.n && f.res[r].status == RMQ_OK && f.res[r].bytes;
        if (served && f.res[r].out_pos == hi && hi > lo) {
          hi += f.res[r].bytes;
          continue;
        }
        if (hi > lo) HIP_TRY(hipMemcpyAsync(f.out + lo, f.d_out + lo, hi - lo, hipMemcpyDeviceToHost, e->fetch_out_s));
        lo = hi = served ? f.res[r].out_pos : 0;
        if (served) hi += f.res[r].bytes;
      }
      HIP_TRY(hipEventRecord(f.ev_copy, e->fetch_out_s));
    } else {
      f.phase = 3;  // nothing to copy
    }
  }
  if (f.phase == 2) {
    const int rc = fetch_await(f.ev_copy, wait);
    if (rc) return rc;
  }
  if (bytes_used) *bytes_used = __atomic_load_n(f.need, __ATOMIC_ACQUIRE);
  f.phase = 0;
  f.ticket = 0;
  return f.rc;
}

// A fetch call as its caller gave it: what the ten entry points pass on, null or 0 for what theirs
// does not take.
struct FetchCall {
  const rmq_fetch_req* reqs;
  const uint64_t* offsets;    // the requests' explicit offsets (rmq_fetch_at, FORMAT.md §7), or null: none
  const uint32_t* max_bytes;  // the requests' byte budgets (rmq_fetch_bytes, FORMAT.md §7), or null: none
  uint32_t n, mem;  // mem, the raw word: the memory kind and the RMQ_FETCH_* flags of the call
  uint8_t* out;
  uint64_t out_cap;
  rmq_fetch_res* res;
  uint64_t *rec_row, *rec_pos, rec_cap;  // the record table (rmq_fetch_table, FORMAT.md §7), or null, null, 0: none
  bool sync;
};

// What the steps of fetch_issue decide about a call, each field set by one step for the later ones.
struct FetchPlan {
  // fetch_check: the memory kind alone, the call's flags (fill: FORMAT.md §7 "Filling a bounded output")
  uint32_t mem = 0;
  bool rows_pinned = false, rows_dev = false, fill = false, table = false;
  // fetch_scan_flags: the OR of the rows' flags
  bool any = false, replica = false, verify = false;
  // fetch_stage: the rows (h_rs: with DMA, the result rows' host copy), words, output and table arrays
  // the kernels read and write
  bool dma = false, dma_in = false;
  void *d_rq = nullptr, *d_rs = nullptr, *h_rs = nullptr;
  const uint32_t* d_bud = nullptr;
  const uint64_t* d_at = nullptr;
  uint8_t* d_out = nullptr;
  uint64_t *d_trow = nullptr, *d_tpos = nullptr;

  // The ticket is a plain resolve + gather pair: nothing of its own runs between or after the two
  // kernels, so they may be the kernels of several tickets at once (held back, fetch_launch) or run
  // again and again under the profiler with dispatch spans (fetch_kernels). Not so a ticket
  //  - that commits: each run would commit again and the next would read from the committed offset,
  //    and the spans' events were measured to hold the second kernel ~10 us behind the first, which
  //    its one run would carry;
  //  - with an RMQ_FETCH_VERIFY request: its third kernel follows its own gather and rewrites the
  //    rows the gather wrote;
  //  - with byte budgets: its trim kernel runs between its own resolve and gather;
  //  - that fills its output: its fill kernel runs before its own gather;
  //  - with a record table: its table kernels follow its own gather and verify, fed by its rows once.
  bool plain_pair() const { return !any && !verify && !d_bud && !fill && !table; }
};

// Step 1, the argument checks: nothing of the engine is read, nothing runs.
int fetch_check(const FetchCall& c, FetchPlan& p) {
  p.table = c.rec_row != nullptr;
  if (!c.rec_row && (c.rec_pos || c.rec_cap)) return RMQ_EINVAL;
  if (!c.rec_pos && c.rec_cap) return RMQ_EINVAL;  // (rec_pos null with rec_cap 0: a size probe)
  if ((c.mem & 3u) == RMQ_MEM_DEVICE &&
      ((reinterpret_cast<uintptr_t>(c.rec_row) | reinterpret_cast<uintptr_t>(c.rec_pos)) & 7u))
    return RMQ_EINVAL;
  p.rows_pinned = (c.mem & RMQ_FETCH_PINNED_ROWS) != 0;
  p.rows_dev = (c.mem & RMQ_FETCH_DEVICE_ROWS) != 0;
  p.fill = (c.mem & RMQ_FETCH_FILL) != 0;
  p.mem = c.mem & ~(RMQ_FETCH_PINNED_ROWS | RMQ_FETCH_DEVICE_ROWS | RMQ_FETCH_FILL);
  if (p.rows_dev && (p.rows_pinned || p.mem != RMQ_MEM_DEVICE)) return RMQ_EINVAL;  // (output on the device too)
  if (p.rows_dev && (reinterpret_cast<uintptr_t>(c.max_bytes) & 3u)) return RMQ_EINVAL;
  if (p.rows_dev && (reinterpret_cast<uintptr_t>(c.offsets) & 7u)) return RMQ_EINVAL;
  if ((c.n && (!c.reqs || !c.res)) || (p.mem != RMQ_MEM_HOST && p.mem != RMQ_MEM_DEVICE)) return RMQ_EINVAL;
  if (c.out_cap && !c.out) return RMQ_EINVAL;
  if (p.mem == RMQ_MEM_DEVICE && (reinterpret_cast<uintptr_t>(c.out) & 15u)) return RMQ_EINVAL;
  return RMQ_OK;
}

// Step 2: every slot taken: complete the oldest into its caller's arrays, keep its result.
int fetch_retire(rmq_engine* e, rmq_engine::FetchSlot& f) {
  if (!f.ticket) return RMQ_OK;
  uint64_t used = 0;
  const uint64_t old = f.ticket;
  const int rc = fetch_slot_step(e, f, true, &used);
  if (rc < 0 && rc != RMQ_ENOSPC) return rc;
  e->fetch_done.push_back({old, (uint64_t)(int64_t)rc, used});
  return RMQ_OK;
}

// Step 3, the rows' flags: known flags only, one committing request per (partition, consumer).
int fetch_scan_flags(rmq_engine* e, const FetchCall& c, FetchPlan& p) {
  if (p.rows_dev) return RMQ_OK;  // (device rows: never read here; their flags are ignored)
  // the OR of every row's flags word (the high half of its second 8-byte word), four rows per
  // step with no early exit: 16,384 rows in a few us instead of a branch per row
  static_assert(sizeof(rmq_fetch_req) == 16 && offsetof(rmq_fetch_req, flags) == 12, "request rows are four words");
  typedef uint64_t __attribute__((__may_alias__)) u64a;
  const u64a* w = reinterpret_cast<const u64a*>(c.reqs);
  uint64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  uint32_t r = 0;
  for (; r + 4 <= c.n; r += 4) {
    a0 |= w[2 * r + 1];
    a1 |= w[2 * r + 3];
    a2 |= w[2 * r + 5];
    a3 |= w[2 * r + 7];
  }
  for (; r < c.n; ++r) a0 |= w[2 * r + 1];
  const uint32_t fl = (uint32_t)((a0 | a1 | a2 | a3) >> 32);
  if (fl & ~(RMQ_FETCH_COMMIT | RMQ_FETCH_REPLICA | RMQ_FETCH_VERIFY)) return RMQ_EINVAL;
  p.any = (fl & RMQ_FETCH_COMMIT) != 0;
  p.replica = (fl & RMQ_FETCH_REPLICA) != 0;
  p.verify = (fl & RMQ_FETCH_VERIFY) != 0;
  if (!p.any) return RMQ_OK;
  const size_t slots = (size_t)e->cfg.num_partitions * e->cfg.max_consumers;
  if (e->fetch_stamp.size() != slots) {
    e->fetch_stamp.assign(slots, 0u);
    e->fetch_stamp_rep.assign(e->cfg.num_partitions, 0u);
    e->fetch_gen = 0;
  }
  if (++e->fetch_gen == 0) {
    std::fill(e->fetch_stamp.begin(), e->fetch_stamp.end(), 0u);
    std::fill(e->fetch_stamp_rep.begin(), e->fetch_stamp_rep.end(), 0u);
    e->fetch_gen = 1;
  }
  for (uint32_t r = 0; r < c.n; ++r) {
    const rmq_fetch_req& q = c.reqs[r];
    if (!(q.flags & RMQ_FETCH_COMMIT) || q.pidx >= e->cfg.num_partitions || q.consumer >= e->cfg.max_consumers)
      continue;
    // a replica read commits the partition's replica cursor: one per partition (any consumer key)
    uint32_t& sl = (q.flags & RMQ_FETCH_REPLICA) ? e->fetch_stamp_rep[q.pidx]
                                                 : e->fetch_stamp[(size_t)q.pidx * e->cfg.max_consumers + q.consumer];
    if (sl == e->fetch_gen) return RMQ_EINVAL;
    sl = e->fetch_gen;
  }
  return RMQ_OK;
}

// Step 4, nothing to fetch: ticket tk completes at once.
int fetch_complete_empty(rmq_engine* e, const FetchCall& c, const FetchPlan& p, uint64_t tk) {
  if (p.table && p.mem == RMQ_MEM_HOST) c.rec_row[0] = 0;  // (rec_row has n + 1 words)
  if (p.table && p.mem == RMQ_MEM_DEVICE) HIP_TRY(hipMemset(c.rec_row, 0, 8));
  e->fetch_done.push_back({tk, (uint64_t)(int64_t)RMQ_OK, 0});
  return RMQ_OK;
}

// Step 5a, the rows. Host rows are page-locked: the caller's own (RMQ_FETCH_PINNED_ROWS, if the
// runtime maps them), else the slot's staging rows. The kernels read and write them in place across
// PCIe (no copy either way: the lowest latency for one call), or (RMQ_FETCH_DMA, asynchronous calls
// by default) the request rows go to the slot's device rows by DMA on the copy stream and the
// result rows come back by DMA on the result stream, so the kernels touch device memory only
// and a burst's copies overlap the other fetches' kernels.
void fetch_stage_rows(rmq_engine* e, rmq_engine::FetchSlot& f, const FetchCall& c, FetchPlan& p) {
  if (p.rows_dev) {
    p.d_rq = const_cast<rmq_fetch_req*>(c.reqs);
    p.d_rs = c.res;
  } else if (p.rows_pinned && (hipHostGetDevicePointer(&p.d_rq, const_cast<rmq_fetch_req*>(c.reqs), 0) != hipSuccess ||
                               hipHostGetDevicePointer(&p.d_rs, c.res, 0) != hipSuccess)) {
    (void)hipGetLastError();
    p.rows_pinned = false;  // not mapped: staged like ordinary rows
  }
  if (!p.rows_pinned && !p.rows_dev) {
    std::memcpy(f.h_req, c.reqs, (size_t)c.n * sizeof(rmq_fetch_req));
    p.d_rq = f.h_req;
    p.d_rs = f.h_res;
  }
  p.dma = !p.rows_dev && (e->knob.fetch_dma >= 2 || (e->knob.fetch_dma == 1 && !c.sync));
  p.h_rs = p.rows_pinned ? static_cast<void*>(c.res) : static_cast<void*>(f.h_res);
  p.dma_in = p.dma && e->knob.fetch_dma_in;
}

// Step 5b, a word per request (the byte budgets, the explicit offsets). Host rows: copied now into
// the slot's page-locked words *h (the caller's array is its own again when the call returns), which
// the kernels read in place, or which go to the device words *d with the request rows
// (RMQ_FETCH_DMA); words that all say `none` are no words: null. Device rows: read where they are.
// (*h and *d are made by the slot's first call that needs them: a slot that never sees one holds the
// scratch it always held; fetch_slot_drop frees them when the slot grows.)
template <typename T>
int fetch_stage_words(rmq_engine* e, const rmq_engine::FetchSlot& f, const FetchPlan& p, const T* src, uint32_t n,
                      T none, T** h, T** d, const T** use) {
  *use = p.rows_dev ? src : nullptr;
  if (!src || p.rows_dev) return RMQ_OK;
  if (!*h) HIP_TRY(hipHostMalloc((void**)h, (size_t)f.cap * sizeof(T), 0));
  if (!*d && p.dma_in) {
    const int rc = fetch_alloc((void**)d, (size_t)f.cap * sizeof(T));
    if (rc) return rc;
  }
  T some = 0;
  for (uint32_t r = 0; r < n; ++r) some |= ((*h)[r] = src[r]) ^ none;
  if (!some) return RMQ_OK;
  *use = *h;
  if (p.dma_in) {
    HIP_TRY(hipMemcpyAsync(*d, *h, (size_t)n * sizeof(T), hipMemcpyHostToDevice, e->copy_s));
    *use = *d;
  }
  return RMQ_OK;
}

// Step 5c, the record table's chunk words, and the device staging of a host table: made by the
// slot's first table call, or its first with host arrays; the staged rec_pos grows as the staged
// output.
int fetch_stage_table(rmq_engine::FetchSlot& f, const FetchCall& c, FetchPlan& p) {
  p.d_trow = c.rec_row;
  p.d_tpos = c.rec_pos;
  if (!p.table) return RMQ_OK;
  int rc = f.d_tsum ? RMQ_OK : fetch_alloc((void**)&f.d_tsum, (size_t)f.csum_lines * 8);
  if (rc || p.mem != RMQ_MEM_HOST) return rc;
  if (!f.d_trow) {
    rc = fetch_alloc((void**)&f.d_trow, ((size_t)f.cap + 1) * 8);
    if (rc) return rc;
  }
  if (c.rec_cap > (1ull << 60)) return RMQ_ENOMEM;
  rc = fetch_grow((void**)&f.d_tpos, &f.tpos_alloc, c.rec_cap, 8);
  if (rc) return rc;
  p.d_trow = f.d_trow;
  p.d_tpos = c.rec_pos ? f.d_tpos : nullptr;
  return RMQ_OK;
}

// Step 5: the slot's scratch, then everything the kernels read staged in it.
int fetch_stage(rmq_engine* e, rmq_engine::FetchSlot& f, const FetchCall& c, FetchPlan& p) {
  int rc = fetch_slot_reserve(f, c.n, p.mem == RMQ_MEM_HOST ? c.out_cap : 0, e->main_s);
  if (rc) return rc;
  p.d_out = p.mem == RMQ_MEM_HOST ? (c.out_cap ? f.d_out : nullptr) : c.out;
  fetch_stage_rows(e, f, c, p);
  rc = fetch_stage_words<uint32_t>(e, f, p, c.max_bytes, c.n, 0u, &f.h_bud, &f.d_bud, &p.d_bud);
  if (!rc) rc = fetch_stage_words<uint64_t>(e, f, p, c.offsets, c.n, RMQ_OFFSET_NONE, &f.h_at, &f.d_at, &p.d_at);
  // (the chunk sums a filling call's gather reads: made by the slot's first filling call, as the
  // offset words)
  if (!rc && p.fill && !f.d_csum_fill) rc = fetch_alloc((void**)&f.d_csum_fill, (size_t)f.csum_lines * kCsumStride * 8);
  if (!rc) rc = fetch_stage_table(f, c, p);
  if (rc) return rc;
  if (p.dma_in) {
    HIP_TRY(hipMemcpyAsync(f.d_req, p.rows_pinned ? static_cast<const void*>(c.reqs) : static_cast<const void*>(f.h_req),
                           (size_t)c.n * sizeof(rmq_fetch_req), hipMemcpyHostToDevice, e->copy_s));
    HIP_TRY(hipEventRecord(f.ev_in, e->copy_s));
    p.d_rq = f.d_req;
  }
  if (p.dma) p.d_rs = f.d_res;  // (the gather reads a request's resolve words, then writes its final row there)
  return RMQ_OK;
}

// The resolve's and the gather's arguments, but for the chunk sums' halves (fetch_csum_halves).
FetchArgs fetch_args(const rmq_engine* e, const rmq_engine::FetchSlot& f, const FetchCall& c, const FetchPlan& p) {
  FetchArgs a{};
  a.st = e->st;
  a.req = static_cast<const uint32_t*>(p.d_rq);
  a.req_dev = f.d_req;
  a.res = f.d_res;
  a.res_host = static_cast<uint64_t*>(p.d_rs);
  a.aux = f.d_aux;
  a.cpre = f.d_cpre;
  a.csum_lines = f.csum_lines;
  a.out = p.d_out;
  a.out_cap = c.out_cap;
  a.need_host = f.need_dev;
  a.n = c.n;
  // (a ticket with an RMQ_FETCH_VERIFY request: the verify kernel commits, after its verdicts)
  a.commits = p.any && !p.verify ? 1u : 0u;
  a.replica = p.replica ? 1u : 0u;
  a.at = p.d_at;
  return a;
}

// A run of the slot's kernels adds into one half of its chunk sums and zeroes the other for the next.
void fetch_csum_halves(rmq_engine::FetchSlot& f, FetchArgs& a) {
  const size_t half = (size_t)f.csum_lines * kCsumStride;
  a.csum = f.d_csum + half * f.csum_par;
  a.csum_next = f.d_csum + half * (f.csum_par ^ 1u);
  f.csum_par ^= 1u;
}

// One run of the ticket's resolve and gather (ev: their dispatch spans), with the trim (budgets) or
// the fill (a filling call) between them.
int fetch_run(rmq_engine* e, rmq_engine::FetchSlot& f, const FetchCall& c, const FetchPlan& p, FetchArgs& a,
              hipEvent_t* ev) {
  fetch_csum_halves(f, a);
  if (p.d_bud || p.fill) {
    FetchTrimArgs t{};
    t.st = e->st;
    t.budget = p.d_bud;
    t.req_dev = f.d_req;
    t.res = f.d_res;
    t.aux = f.d_aux;
    t.cpre = f.d_cpre;
    t.csum = a.csum;
    t.n = c.n;
    if (p.fill) {
      FetchFillArgs ff{};
      ff.t = t;
      ff.csum_out = f.d_csum_fill;
      ff.out_cap = c.out_cap;
      ff.verify = p.verify ? 1u : 0u;
      launch_fetch_fill(a, ff, e->main_s);
    } else {
      launch_fetch_budget(a, t, e->main_s);
    }
  } else {
    launch_fetch(a, e->main_s, ev);
  }
  HIP_TRY(hipGetLastError());
  return RMQ_OK;
}

// The flagged slices checked in the output, then the ticket's commits.
int fetch_verify(rmq_engine* e, const rmq_engine::FetchSlot& f, const FetchPlan& p, const FetchArgs& a) {
  FetchVerifyArgs v{};
  v.st = e->st;
  v.req_dev = f.d_req;
  v.rows = a.res_host;
  v.out = p.d_out;
  v.crc = e->d_crc;
  v.n = a.n;
  v.commits = p.any ? 1u : 0u;
  v.replica = a.replica;
  launch_fetch_verify(v, audit_wgs(e), e->main_s);
  HIP_TRY(hipGetLastError());
  return RMQ_OK;
}

// A span of rmq_profile_query's kernel k opens on the pipeline stream: *end is recorded behind it.
hipError_t fetch_prof_open(rmq_engine* e, int k, hipEvent_t* end) {
  const hipEvent_t begin = pool_event(e);
  *end = pool_event(e);
  e->prof[k].push_back({begin, *end});
  return hipEventRecord(begin, e->main_s);
}

// The record table from the final rows (profile kernel 9: the span of its kernels).
int fetch_table(rmq_engine* e, const rmq_engine::FetchSlot& f, const FetchCall& c, const FetchPlan& p, const FetchArgs& a) {
  FetchTableArgs t{};
  t.rows = a.res_host;
  t.out = p.d_out;
  t.rec_row = p.d_trow;
  t.rec_pos = p.d_tpos;
  t.rec_cap = c.rec_cap;
  t.tsum = f.d_tsum;
  t.need_host = f.tneed_dev;
  t.n = c.n;
  hipEvent_t t1 = nullptr;
  if (e->profile) HIP_TRY(fetch_prof_open(e, 9, &t1));
  launch_fetch_table(t, audit_wgs(e), e->main_s);
  HIP_TRY(hipGetLastError());
  if (e->profile) HIP_TRY(hipEventRecord(t1, e->main_s));
  return RMQ_OK;
}

// The ticket's kernels on the pipeline stream. Profiling (kernel 3: the first run's dispatch spans;
// 4: every run) replays the kernels of a plain pair back to back; anything else runs once, without
// spans.
int fetch_kernels(rmq_engine* e, rmq_engine::FetchSlot& f, const FetchCall& c, const FetchPlan& p, FetchArgs& a) {
  const uint32_t runs = e->profile && p.plain_pair() ? e->fetch_replay : 1u;
  const bool spans = e->profile && p.plain_pair();
  hipEvent_t ev[4] = {}, r1 = nullptr;
  if (spans) {
    for (hipEvent_t& x : ev) x = pool_event(e);
    for (int k = 0; k < 2; ++k) e->prof[3].push_back({ev[2 * k], ev[2 * k + 1]});
  }
  if (e->profile) {
    e->prof_fetch_runs += runs;
    HIP_TRY(fetch_prof_open(e, 4, &r1));
  }
  int rc = RMQ_OK;
  for (uint32_t k = 0; k < runs && !rc; ++k) rc = fetch_run(e, f, c, p, a, spans && k == 0 ? ev : nullptr);
  if (!rc && p.verify) rc = fetch_verify(e, f, p, a);
  if (!rc && p.table) rc = fetch_table(e, f, c, p, a);
  if (rc) return rc;
  if (e->profile) HIP_TRY(hipEventRecord(r1, e->main_s));
  return RMQ_OK;
}

// Step 6, under the engine lock (not EngineLock: this decides about the held-back fetches): order
// the ticket against the append pipeline without flushing it, on the pipeline's stream, after the
// last launch issued so far and before the next, so no ring bytes or log starts it reads change
// under it.
int fetch_launch(rmq_engine* e, rmq_engine::FetchSlot& f, const FetchCall& c, const FetchPlan& p) {
  std::lock_guard<std::mutex> g(e->mu);
  // an asynchronous plain pair waits to go with the next ones (up to kFetchBatch tickets in one
  // resolve + gather pair: the requests of different tickets never depend on one another); anything
  // else launches the held ones first, then itself. Nor is a call held that passes an offsets array:
  // only the single-ticket resolve reads them; an array whose entries are all RMQ_OFFSET_NONE is read
  // by nothing and launches the plain resolve, but FORMAT.md §7 says so of every call with
  // offsets != NULL.
  const bool hold = !c.sync && p.plain_pair() && !c.offsets && !p.dma && !e->profile && e->knob.fetch_coalesce > 1;
  int rc = hold ? RMQ_OK : fetch_flush(e);
  if (rc) return rc;
  if (p.dma_in) HIP_TRY(hipStreamWaitEvent(e->main_s, f.ev_in, 0));
  rc = hold ? RMQ_OK : late_retention(e);  // (the log starts the fetch reads: every batch applied so far retained)
  if (rc) return rc;
  FetchArgs a = fetch_args(e, f, c, p);
  if (hold) {  // (the completion event: recorded when fetch_flush launches the kernels)
    fetch_csum_halves(f, a);
    f.args = a;
    f.pending = true;
    e->fpend.push_back(e->fslot_next);
    return e->fpend.size() >= std::min<uint32_t>(kFetchBatch, e->knob.fetch_coalesce) ? fetch_flush(e) : RMQ_OK;
  }
  rc = fetch_kernels(e, f, c, p, a);
  if (rc) return rc;
  if (p.dma) {  // the result rows to the host behind the kernels, off the pipeline stream
    HIP_TRY(hipEventRecord(f.ev_k, e->main_s));
    HIP_TRY(hipStreamWaitEvent(e->fetch_out_s, f.ev_k, 0));
    HIP_TRY(hipMemcpyAsync(p.h_rs, f.d_res, (size_t)c.n * sizeof(rmq_fetch_res), hipMemcpyDeviceToHost, e->fetch_out_s));
    HIP_TRY(hipEventRecord(f.ev, e->fetch_out_s));
  } else {
    HIP_TRY(hipEventRecord(f.ev, e->main_s));  // kernels done: result rows and bytes needed in place
  }
  return RMQ_OK;
}

// Step 7: ticket tk is in flight in the slot, what rmq_fetch_poll needs to complete it kept.
void fetch_record(rmq_engine* e, rmq_engine::FetchSlot& f, const FetchCall& c, const FetchPlan& p, uint64_t tk) {
  f.rows_pinned = p.rows_pinned || p.rows_dev;  // (no copy of the rows at completion)
  f.ticket = tk;
  f.phase = 1;
  f.rc = RMQ_OK;
  f.n = c.n;
  f.mem = p.mem;
  f.out = c.out;
  f.out_cap = c.out_cap;
  f.res = c.res;
  f.table = p.table;
  f.t_row = p.table && p.mem == RMQ_MEM_HOST ? c.rec_row : nullptr;
  f.t_pos = c.rec_pos;
  f.t_cap = c.rec_cap;
  e->fslot_next = (e->fslot_next + 1) % rmq_engine::kFetchSlots;
}

// Issue a fetch into the next slot: its kernels on the pipeline stream, an event after them.
int fetch_issue(rmq_engine* e, const FetchCall& c, uint64_t* ticket) {
  if (!e || !ticket) return RMQ_EINVAL;
  FetchPlan p;
  int rc = fetch_check(c, p);
  if (rc) return rc;
  std::lock_guard<std::mutex> fg(e->fetch_mu);
  HIP_TRY(hipSetDevice(e->device));
  rmq_engine::FetchSlot& f = e->fslot[e->fslot_next];
  rc = fetch_retire(e, f);
  if (!rc) rc = fetch_scan_flags(e, c, p);
  if (rc) return rc;
  const uint64_t tk = ++e->fetch_seq;
  if (!c.n) {
    rc = fetch_complete_empty(e, c, p, tk);
    if (rc) return rc;
  } else {
    rc = fetch_stage(e, f, c, p);
    if (!rc) rc = fetch_launch(e, f, c, p);
    if (rc) return rc;
    fetch_record(e, f, c, p, tk);
  }
  while (e->fetch_done.size() > 256) e->fetch_done.pop_front();
  *ticket = tk;
  return RMQ_OK;
}

// The synchronous calls: issue, then wait for the ticket (a call with nothing to fetch and no table
// to clear is done at once).
int fetch_sync(rmq_engine* e, const FetchCall& c, uint64_t* bytes_used) {
  if (bytes_used) *bytes_used = 0;
  if (!e) return RMQ_EINVAL;
  if (!c.n && !c.rec_row && !c.rec_pos && !c.rec_cap) return RMQ_OK;
  uint64_t t = 0;
  const int rc = fetch_issue(e, c, &t);
  return rc ? rc : rmq_fetch_poll(e, t, 1, bytes_used);
}

}  // namespace

// The asynchronous fetches held back (fetch_launch) as ONE resolve + gather pair (kFetchBatch tickets
// at most), each ticket's completion event after it. Called (under mu) by the next fetch that cannot
// join them, by every other call that takes the engine lock (EngineLock: whatever it issues on the
// pipeline stream stays ordered after the fetches issued before it), and by a poll of a held ticket.
int fetch_flush(rmq_engine* e) {
  if (e->fpend.empty()) return RMQ_OK;
  int rc = late_retention(e);
  if (rc) return rc;
  FetchArgs t[kFetchBatch];
  uint32_t nt = 0;
  for (uint32_t i : e->fpend) t[nt++] = e->fslot[i].args;
  launch_fetch_batch(t, nt, e->main_s);
  HIP_TRY(hipGetLastError());
  for (uint32_t i : e->fpend) {
    HIP_TRY(hipEventRecord(e->fslot[i].ev, e->main_s));
    e->fslot[i].pending = false;
  }
  e->fpend.clear();
  return RMQ_OK;
}

void fetch_free(rmq_engine* e) {
  for (rmq_engine::FetchSlot& f : e->fslot) {
    fetch_slot_drop(f);
    if (f.d_out) hipFree(f.d_out);
    if (f.d_tpos) hipFree(f.d_tpos);
    for (hipEvent_t ev : {f.ev, f.ev_copy, f.ev_in, f.ev_k})
      if (ev) hipEventDestroy(ev);
  }
}

}  // namespace rmq

extern "C" {

int rmq_fetch_poll(rmq_engine* e, uint64_t ticket, uint32_t wait, uint64_t* bytes_used) {
  if (!e || !ticket) return RMQ_EINVAL;
  std::lock_guard<std::mutex> fg(e->fetch_mu);
  if (bytes_used) *bytes_used = 0;
  for (rmq_engine::FetchSlot& f : e->fslot)
    if (f.ticket == ticket) {
      HIP_TRY(hipSetDevice(e->device));
      return fetch_slot_step(e, f, wait != 0, bytes_used);
    }
  for (auto it = e->fetch_done.begin(); it != e->fetch_done.end(); ++it)
    if ((*it)[0] == ticket) {
      const int rc = (int)(int64_t)(*it)[1];
      if (bytes_used) *bytes_used = (*it)[2];
      e->fetch_done.erase(it);
      return rc;
    }
  return RMQ_EINVAL;
}

int rmq_fetch(rmq_engine* e, const rmq_fetch_req* reqs, uint32_t n, uint32_t mem, uint8_t* out,
              uint64_t out_cap, rmq_fetch_res* res, uint64_t* bytes_used) {
  return fetch_sync(e, {reqs, nullptr, nullptr, n, mem, out, out_cap, res, nullptr, nullptr, 0, true}, bytes_used);
}

int rmq_fetch_async(rmq_engine* e, const rmq_fetch_req* reqs, uint32_t n, uint32_t mem, uint8_t* out,
                    uint64_t out_cap, rmq_fetch_res* res, uint64_t* ticket) {
  return fetch_issue(e, {reqs, nullptr, nullptr, n, mem, out, out_cap, res, nullptr, nullptr, 0, false}, ticket);
}

int rmq_fetch_bytes(rmq_engine* e, const rmq_fetch_req* reqs, const uint32_t* max_bytes, uint32_t n,
                    uint32_t mem, uint8_t* out, uint64_t out_cap, rmq_fetch_res* res, uint64_t* bytes_used) {
  return fetch_sync(e, {reqs, nullptr, max_bytes, n, mem, out, out_cap, res, nullptr, nullptr, 0, true}, bytes_used);
}

int rmq_fetch_bytes_async(rmq_engine* e, const rmq_fetch_req* reqs, const uint32_t* max_bytes, uint32_t n,
                          uint32_t mem, uint8_t* out, uint64_t out_cap, rmq_fetch_res* res, uint64_t* ticket) {
  return fetch_issue(e, {reqs, nullptr, max_bytes, n, mem, out, out_cap, res, nullptr, nullptr, 0, false}, ticket);
}

int rmq_fetch_at(rmq_engine* e, const rmq_fetch_req* reqs, const uint64_t* offsets, const uint32_t* max_bytes,
                 uint32_t n, uint32_t mem, uint8_t* out, uint64_t out_cap, rmq_fetch_res* res, uint64_t* bytes_used) {
  return fetch_sync(e, {reqs, offsets, max_bytes, n, mem, out, out_cap, res, nullptr, nullptr, 0, true}, bytes_used);
}

int rmq_fetch_at_async(rmq_engine* e, const rmq_fetch_req* reqs, const uint64_t* offsets, const uint32_t* max_bytes,
                       uint32_t n, uint32_t mem, uint8_t* out, uint64_t out_cap, rmq_fetch_res* res, uint64_t* ticket) {
  return fetch_issue(e, {reqs, offsets, max_bytes, n, mem, out, out_cap, res, nullptr, nullptr, 0, false}, ticket);
}

int rmq_fetch_table(rmq_engine* e, const rmq_fetch_req* reqs, const uint64_t* offsets, const uint32_t* max_bytes,
                    uint32_t n, uint32_t mem, uint8_t* out, uint64_t out_cap, rmq_fetch_res* res,
                    uint64_t* rec_row, uint64_t* rec_pos, uint64_t rec_cap, uint64_t* bytes_used) {
  return fetch_sync(e, {reqs, offsets, max_bytes, n, mem, out, out_cap, res, rec_row, rec_pos, rec_cap, true}, bytes_used);
}

int rmq_fetch_table_async(rmq_engine* e, const rmq_fetch_req* reqs, const uint64_t* offsets, const uint32_t* max_bytes,
                          uint32_t n, uint32_t mem, uint8_t* out, uint64_t out_cap, rmq_fetch_res* res,
                          uint64_t* rec_row, uint64_t* rec_pos, uint64_t rec_cap, uint64_t* ticket) {
  return fetch_issue(e, {reqs, offsets, max_bytes, n, mem, out, out_cap, res, rec_row, rec_pos, rec_cap, false}, ticket);
}

}  // extern "C"
