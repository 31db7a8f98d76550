// audit.cpp — the audit calls of the C-ABI: rmq_scrub, rmq_repair, rmq_reindex, rmq_repair_remote and
// rmq_restore (FORMAT.md §10), each its own sequence of kernels on the drained pipeline stream.
//
// They share no state with append or fetch: each takes the engine lock, drains, grows its device
// buffers on demand (rmq_engine::Audit, rmq_engine::Restore), launches, waits and decodes the result
// rows on the host. The steps they have in common are the file-local helpers below.
#include "engine_internal.hpp"
#include "restore_check.hpp"

using namespace rmq;

namespace rmq {

// Everything the audit calls grew: rmq_engine::Audit and rmq_restore's rmq_engine::Restore.
void audit_free(rmq_engine* e) {
  rmq_engine::Audit& B = e->au;
  void* bufs[] = {B.tbase, B.rows, B.verdict, B.counts, B.gaps, B.scratch, B.rcounts};
  for (void* p : bufs)
    if (p) hipFree(p);
  B = rmq_engine::Audit();
  rmq_engine::Restore& R = e->rs;
  void* rbufs[] = {R.buf, R.tab, R.items, R.rbase, R.key};
  for (void* p : rbufs)
    if (p) hipFree(p);
  R = rmq_engine::Restore();
}

namespace {

// The bound on the tasks of a range (a verdict per task): a partition has at most ring bytes /
// interval + 2 segments on each of its local slots, RF at the most.
uint64_t audit_tasks(const rmq_engine* e, uint32_t first, uint32_t n) {
  uint64_t tasks = 0;
  for (uint32_t p = first; p < first + n; ++p)
    tasks += e->cfg.replication_factor * ((ring_bytes(e->ring[p]) >> e->st.interval_log2) + 2ull);
  return tasks;
}

// The prologue under the engine lock: the range check, nothing to do for an empty range (unless the
// call is collective: a rank of rmq_repair_remote with n = 0 drains and serves too), then the drain
// (fetches run on the pipeline stream: the drain waits for them too). *go: the call goes on.
int audit_begin(rmq_engine* e, uint32_t first, uint32_t n, bool* go, bool collective = false) {
  *go = false;
  const uint32_t P = e->cfg.num_partitions;
  if (first > P || n > P - first) return RMQ_ENOPART;
  if (!n && !collective) return RMQ_OK;
  const int rc = begin_call(e, drain);
  *go = rc == RMQ_OK;
  return rc;
}

// The plan's scan and the result rows of a range of n partitions, and a verdict byte per task of the
// bound (tasks = 0: none, rmq_scrub).
int audit_buffers(rmq_engine* e, uint32_t n, uint64_t tasks) {
  rmq_engine::Audit& B = e->au;
  int rc = grow(&B.tbase, &B.tbase_cap, (uint64_t)n + 1);
  if (!rc) rc = grow(&B.rows, &B.rows_cap, 4ull * n);
  if (!rc && tasks) rc = grow(&B.verdict, &B.verdict_cap, tasks);
  return rc;
}

ScrubArgs scrub_args(const rmq_engine* e, uint32_t first, uint32_t n) {
  ScrubArgs a{};
  a.st = e->st;
  a.crc = e->d_crc;
  a.tbase = e->au.tbase;
  a.rows = e->au.rows;
  a.first = first;
  a.n = n;
  return a;
}

// The repair's buffers (an empty range, which only rmq_repair_remote gets this far with, grows none)
// and its arguments.
int repair_args(rmq_engine* e, uint32_t first, uint32_t n, uint32_t flags, uint64_t tasks, RepairArgs* a) {
  rmq_engine::Audit& B = e->au;
  int rc = n ? audit_buffers(e, n, tasks) : RMQ_OK;
  if (!rc && n) rc = grow(&B.counts, &B.counts_cap, 3ull * n);
  a->s = scrub_args(e, first, n);
  a->verdict = B.verdict;
  a->counts = B.counts;
  a->write = (flags & RMQ_REPAIR_DRY_RUN) ? 0u : 1u;
  return rc;
}

// A call's region of rmq_profile_query's kernel k: an event before its first kernel to one after its
// last, so the second is recorded again after every later batch of kernels. No events with
// profiling off. (A launch_scrub inside another call belongs to that call's region, not to kernel 2.)
struct ProfRegion {
  hipStream_t s = nullptr;
  hipEvent_t r1 = nullptr;
  bool on = false;
  int open(rmq_engine* e, int k, hipStream_t stream) {
    s = stream;
    on = e->profile != 0;
    if (!on) return RMQ_OK;
    hipEvent_t r0 = pool_event(e);
    r1 = pool_event(e);
    e->prof[k].push_back({r0, r1});
    HIP_TRY(hipEventRecord(r0, s));
    return RMQ_OK;
  }
  int mark() {
    if (on) HIP_TRY(hipEventRecord(r1, s));
    return RMQ_OK;
  }
  // after a batch of launches: their error and the region's end behind them; sync() then waits
  int launched() {
    HIP_TRY(hipGetLastError());
    return mark();
  }
  int sync() {
    const int rc = launched();
    return rc ? rc : stream_wait(s);
  }
};

// A failure key is offset << 5 | slot << 2 | kind (kernels.hpp); rmq_restore's keys have no slot.
uint64_t key_offset(uint64_t key) { return key >> 5; }
uint32_t key_replica(uint64_t key) { return (uint32_t)(key >> 2) & 7u; }
uint32_t key_kind(uint64_t key) { return (uint32_t)key & 3u; }

bool any_corrupt(const std::vector<uint64_t>& rows, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    if (rows[4ull * i] != kScrubClean) return true;
  return false;
}

// The verdict fields every result struct of a scrub row has, from the row {key, records ok, bytes ok,
// local replica slots}; the caller has cleared x and sets its own counters.
template <typename X>
void put_verdict(X& x, const uint64_t* row) {
  const uint64_t key = row[0];
  const bool clean = key == kScrubClean;
  x.replicas = (uint32_t)row[3];
  x.bad_offset = clean ? RMQ_OFFSET_NONE : key_offset(key);
  x.bad_replica = clean ? 0u : key_replica(key);
  x.bad_kind = clean ? 0u : key_kind(key);
  x.status = clean ? RMQ_OK : RMQ_ECORRUPT;
}

}  // namespace
}  // namespace rmq

extern "C" {

int rmq_scrub(rmq_engine* e, uint32_t first, uint32_t n, rmq_scrub_res* res) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  bool go;
  int rc = audit_begin(e, first, n, &go);
  if (!go) return rc;
  rc = audit_buffers(e, n, 0);
  if (rc) return rc;
  const ScrubArgs a = scrub_args(e, first, n);
  ProfRegion pr;
  rc = pr.open(e, 2, e->main_s);
  if (rc) return rc;
  // the tasks are counted on the device (the plan), so the verify grid is a fixed few workgroups
  // per CU whose waves stride over them
  launch_scrub(a, audit_wgs(e), e->main_s);
  rc = pr.sync();
  if (rc) return rc;
  std::vector<uint64_t> rows((size_t)n * 4);
  rc = read_words(rows, e->au.rows);
  if (rc) return rc;
  for (uint32_t i = 0; res && i < n; ++i) {
    rmq_scrub_res& x = res[i];
    std::memset(&x, 0, sizeof x);
    x.records_ok = rows[4ull * i + 1];
    x.bytes_ok = rows[4ull * i + 2];
    put_verdict(x, &rows[4ull * i]);
  }
  return any_corrupt(rows, n) ? RMQ_ECORRUPT : RMQ_OK;
}

// Scan (the scrub with a verdict per task); if it found corruption, the copy from a clean local slot
// on the same plan, then (unless nothing may be written) the scrub again.
int rmq_repair(rmq_engine* e, uint32_t first, uint32_t n, uint32_t flags, rmq_repair_res* res) {
  if (!e || (flags & ~RMQ_REPAIR_DRY_RUN)) return RMQ_EINVAL;
  EngineLock g(e);
  bool go;
  int rc = audit_begin(e, first, n, &go);
  if (!go) return rc;
  rmq_engine::Audit& B = e->au;
  RepairArgs a{};
  rc = repair_args(e, first, n, flags, audit_tasks(e, first, n), &a);
  if (rc) return rc;
  ProfRegion pr;
  rc = pr.open(e, 5, e->main_s);
  if (rc) return rc;
  launch_repair_scan(a, audit_wgs(e), e->main_s);
  rc = pr.sync();
  if (rc) return rc;
  std::vector<uint64_t> rows((size_t)n * 4), counts((size_t)n * 3, 0);
  rc = read_words(rows, B.rows);
  if (rc) return rc;
  if (any_corrupt(rows, n)) {
    HIP_TRY(hipMemsetAsync(B.counts, 0, counts.size() * 8, e->main_s));
    launch_repair_copy(a, audit_wgs(e), e->main_s);
    if (a.write) launch_scrub(a.s, audit_wgs(e), e->main_s);
    rc = pr.sync();
    if (!rc) rc = read_words(counts, B.counts);
    if (!rc && a.write) rc = read_words(rows, B.rows);  // (a dry run reports the first pass's rows)
    if (rc) return rc;
  }
  for (uint32_t i = 0; res && i < n; ++i) {
    rmq_repair_res& x = res[i];
    std::memset(&x, 0, sizeof x);
    x.segments_repaired = counts[3ull * i];
    x.bytes_repaired = counts[3ull * i + 1];
    x.segments_unrepaired = counts[3ull * i + 2];
    put_verdict(x, &rows[4ull * i]);
  }
  return any_corrupt(rows, n) ? RMQ_ECORRUPT : RMQ_OK;
}

// The repair's scan, then the gaps, the walks and the install of reindex.hip on the same plan, then
// (if an entry changed) the scrub again.
int rmq_reindex(rmq_engine* e, uint32_t first, uint32_t n, uint32_t flags, rmq_reindex_res* res) {
  if (!e || (flags & ~(RMQ_REINDEX_DRY_RUN | RMQ_REINDEX_ALL))) return RMQ_EINVAL;
  EngineLock g(e);
  bool go;
  int rc = audit_begin(e, first, n, &go);
  if (!go) return rc;
  rmq_engine::Audit& B = e->au;
  // a gap and a rebuilt entry per task of the bound at the most (a partition with a local slot has at
  // least as many tasks as live entries plus one)
  const uint64_t tasks = audit_tasks(e, first, n);
  rc = audit_buffers(e, n, tasks);
  if (!rc) rc = grow(&B.gaps, &B.gaps_cap, 2 * tasks);
  if (!rc) rc = grow(&B.scratch, &B.scratch_cap, 2 * tasks);
  if (!rc) rc = grow(&B.rcounts, &B.rcounts_cap, 3ull * n + 1);
  if (rc) return rc;
  ReindexArgs a{};
  a.s = scrub_args(e, first, n);
  a.verdict = B.verdict;
  a.gaps = B.gaps;
  a.scratch = B.scratch;
  a.counts = B.rcounts;
  a.ngaps = reinterpret_cast<uint32_t*>(B.rcounts + (size_t)n * 3);
  a.cap = tasks;  // (>= n: every partition of the range adds at least 2 RF)
  a.all = (flags & RMQ_REINDEX_ALL) ? 1u : 0u;
  a.write = (flags & RMQ_REINDEX_DRY_RUN) ? 0u : 1u;
  RepairArgs ra{};
  ra.s = a.s;
  ra.verdict = B.verdict;
  ProfRegion pr;
  rc = pr.open(e, 8, e->main_s);
  if (rc) return rc;
  std::vector<uint64_t> rows((size_t)n * 4), counts((size_t)n * 3, 0);
  HIP_TRY(hipMemsetAsync(B.rcounts, 0, (counts.size() + 1) * 8, e->main_s));
  launch_repair_scan(ra, audit_wgs(e), e->main_s);
  launch_reindex(a, audit_wgs(e), e->main_s);
  rc = pr.sync();
  if (!rc) rc = read_words(rows, B.rows);
  if (!rc) rc = read_words(counts, B.rcounts);
  if (rc) return rc;
  bool wrote = false;
  for (uint32_t i = 0; i < n && !wrote; ++i) wrote = a.write && counts[3ull * i + 1] != 0;
  if (wrote) {
    launch_scrub(a.s, audit_wgs(e), e->main_s);
    rc = pr.sync();
    if (!rc) rc = read_words(rows, B.rows);
    if (rc) return rc;
  }
  for (uint32_t i = 0; res && i < n; ++i) {
    rmq_reindex_res& x = res[i];
    std::memset(&x, 0, sizeof x);
    x.entries_live = counts[3ull * i];
    x.entries_rewritten = counts[3ull * i + 1];
    x.gaps_unresolved = counts[3ull * i + 2];
    put_verdict(x, &rows[4ull * i]);
  }
  return any_corrupt(rows, n) ? RMQ_ECORRUPT : RMQ_OK;
}

// rmq_repair's scan and local copy, then the rounds over the transport (repair_remote.cpp), then the
// scrub again. Without a transport this is rmq_repair step by step.
int rmq_repair_remote(rmq_engine* e, uint32_t first, uint32_t n, uint32_t flags, rmq_repair_remote_res* res,
                      uint64_t* served) {
  if (!e || (flags & ~RMQ_REPAIR_DRY_RUN)) return RMQ_EINVAL;
  EngineLock g(e);
  if (served) served[0] = served[1] = 0;
  bool go;
  int rc = audit_begin(e, first, n, &go, e->repl != nullptr);
  if (!go) return rc;
  rmq_engine::Audit& B = e->au;
  const uint64_t tasks = audit_tasks(e, first, n);
  RepairArgs a{};
  rc = repair_args(e, first, n, flags, tasks, &a);
  if (rc) return rc;
  ProfRegion pr;
  rc = pr.open(e, 6, e->main_s);
  if (!rc) rc = pr.mark();  // (a rank that launches nothing still has a complete pair)
  if (rc) return rc;
  std::vector<uint64_t> rows((size_t)n * 4), counts((size_t)n * 3, 0), fetched((size_t)n * 2, 0);
  bool corrupt = false;
  if (n) {
    launch_repair_scan(a, audit_wgs(e), e->main_s);
    rc = pr.sync();
    if (!rc) rc = read_words(rows, B.rows);
    if (rc) return rc;
    corrupt = any_corrupt(rows, n);
    if (corrupt) {
      HIP_TRY(hipMemsetAsync(B.counts, 0, counts.size() * 8, e->main_s));
      launch_repair_copy(a, audit_wgs(e), e->main_s);
      rc = pr.launched();
      if (rc) return rc;
    }
  }
  uint64_t sv[2] = {0, 0};
  if (e->repl) {
    rc = repair_remote_rounds(e, corrupt ? &a : nullptr, audit_wgs(e), tasks, fetched.data(), sv);
    if (!rc) rc = pr.mark();
    if (rc) return rc;
  }
  if (served) served[0] = sv[0], served[1] = sv[1];
  if (corrupt) {
    if (a.write) launch_scrub(a.s, audit_wgs(e), e->main_s);
    rc = pr.sync();
    if (!rc) rc = read_words(counts, B.counts);
    if (!rc && a.write) rc = read_words(rows, B.rows);  // (a dry run reports the first pass's rows)
    if (rc) return rc;
  }
  for (uint32_t i = 0; res && i < n; ++i) {
    rmq_repair_remote_res& x = res[i];
    std::memset(&x, 0, sizeof x);
    x.segments_repaired = counts[3ull * i];
    x.bytes_repaired = counts[3ull * i + 1];
    x.segments_fetched = fetched[2ull * i];
    x.bytes_fetched = fetched[2ull * i + 1];
    x.segments_unrepaired = counts[3ull * i + 2] - fetched[2ull * i];  // (a fetched pair had no local donor)
    put_verdict(x, &rows[4ull * i]);
  }
  return any_corrupt(rows, n) ? RMQ_ECORRUPT : RMQ_OK;
}

// Host checks (restore_check.hpp), staging, then verify -> install -> finish on the pipeline stream
// (restore.hip): the verdicts stay on the device between the passes and are read back once.
int rmq_restore(rmq_engine* e, uint32_t n, const rmq_restore_item* items, uint32_t mem, const uint8_t* buf,
                uint64_t buf_bytes, const uint64_t* rec_pos, uint64_t rec_words, uint32_t flags, rmq_restore_res* res) {
  if (!e || (flags & ~RMQ_RESTORE_DRY_RUN) || (n && !items) || (mem != RMQ_MEM_HOST && mem != RMQ_MEM_DEVICE) ||
      (buf_bytes && !buf) || (rec_words && !rec_pos) || (mem == RMQ_MEM_DEVICE && ((uintptr_t)buf & 15u)))
    return RMQ_EINVAL;
  EngineLock g(e);
  if (e->repl) return RMQ_EINVAL;  // a restarted rank restores before it attaches
  if (!n) return RMQ_OK;
  HIP_TRY(hipSetDevice(e->device));
  int rc = drain(e);
  if (rc) return rc;
  const uint32_t P = e->cfg.num_partitions, RF = e->cfg.replication_factor;
  // pristine: log start and end offsets and positions all 0 (the engine is drained: the current set)
  std::vector<uint64_t> so(P), sp(P), eo(P), ep(P);
  rc = read_words(so, e->st.start_off);
  if (!rc) rc = read_words(sp, e->st.start_pos);
  if (!rc) rc = read_words(eo, e->st.leo);
  if (!rc) rc = read_words(ep, e->st.used);
  if (rc) return rc;
  const RestorePlan pl = restore_plan(n, items, P, buf_bytes, rec_words, [&](uint32_t p) {
    RestorePart q;
    q.seg = ring_bytes(e->ring[p]);
    q.pristine = !(so[p] | sp[p] | eo[p] | ep[p]);
    q.local = false;
    for (uint32_t r = 0; r < RF; ++r) q.local = q.local || e->ranks[(size_t)p * RF + r] == e->cfg.rank;
    return q;
  });
  const uint32_t na = (uint32_t)pl.accepted.size();
  std::vector<uint64_t> key(na, kScrubClean);
  if (na) {
    const bool host = mem == RMQ_MEM_HOST;
    rmq_engine::Restore& B = e->rs;
    if (B.items_cap < na) {  // the three per-item arrays share a capacity
      uint64_t c0 = 0, c1 = 0, c2 = 0;
      B.items_cap = 0;
      rc = restore_grow(&B.items, &c0, na);
      if (!rc) rc = restore_grow(&B.rbase, &c1, (uint64_t)na + 1);
      if (!rc) rc = restore_grow(&B.key, &c2, na);
      if (!rc) B.items_cap = na;
    }
    if (!rc) rc = restore_grow(&B.tab, &B.tab_cap, pl.tab_hi - pl.tab_lo);
    if (!rc && host && pl.buf_hi > pl.buf_lo) rc = restore_grow(&B.buf, &B.buf_cap, pl.buf_hi - pl.buf_lo);
    if (rc) return rc;
    std::vector<RestoreItem> di(na);
    for (uint32_t k = 0; k < na; ++k) {
      const rmq_restore_item& it = items[pl.accepted[k]];
      RestoreItem& d = di[k];
      d.first_off = it.first_offset, d.first_pos = it.first_pos, d.count = it.count, d.bytes = it.bytes;
      d.run = host ? B.buf + (it.bytes ? it.buf_pos - pl.buf_lo : 0ull) : buf + it.buf_pos;
      d.tab = B.tab + (it.table_start - pl.tab_lo);
      d.commit = it.commit;
      d.pidx = it.pidx, d.pad = 0;
    }
    hipStream_t s = e->main_s;
    HIP_TRY(hipMemcpyAsync(B.items, di.data(), (size_t)na * sizeof(RestoreItem), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(B.rbase, pl.rbase.data(), ((size_t)na + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(B.key, key.data(), (size_t)na * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(B.tab, rec_pos + pl.tab_lo, (size_t)(pl.tab_hi - pl.tab_lo) * 8, hipMemcpyHostToDevice, s));
    if (host && pl.buf_hi > pl.buf_lo)
      HIP_TRY(hipMemcpyAsync(B.buf, buf + pl.buf_lo, (size_t)(pl.buf_hi - pl.buf_lo), hipMemcpyHostToDevice, s));
    RestoreArgs a{};
    a.st = e->st;
    a.sets[0] = e->sets[0];
    a.sets[1] = e->sets[1];
    a.crc = e->d_crc;
    a.items = B.items;
    a.rbase = B.rbase;
    a.key = B.key;
    a.n = na;
    ProfRegion pr;
    rc = pr.open(e, 7, s);
    if (rc) return rc;
    const uint64_t records = pl.rbase.back();
    launch_restore_verify(a, records, audit_wgs(e), s);
    if (!(flags & RMQ_RESTORE_DRY_RUN)) launch_restore_install(a, records, audit_wgs(e), s);
    rc = pr.launched();
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(key.data(), B.key, (size_t)na * 8, hipMemcpyDeviceToHost, s));
    rc = stream_wait(s);  // (the caller's buffers are free again, and the rows can be written)
    if (rc) return rc;
  }
  std::vector<int32_t> status = pl.status;
  for (uint32_t k = 0; k < na; ++k)
    if (key[k] != kScrubClean) status[pl.accepted[k]] = RMQ_ECORRUPT;
  if (res) {
    for (uint32_t i = 0; i < n; ++i) {
      rmq_restore_res& x = res[i];
      std::memset(&x, 0, sizeof x);
      x.bad_offset = RMQ_OFFSET_NONE;
      x.status = status[i];
    }
    for (uint32_t k = 0; k < na; ++k) {
      rmq_restore_res& x = res[pl.accepted[k]];
      if (key[k] == kScrubClean) {
        x.records = items[pl.accepted[k]].count;
        x.bytes = items[pl.accepted[k]].bytes;
      } else {
        x.bad_offset = key_offset(key[k]);
        x.bad_kind = key_kind(key[k]);
      }
    }
  }
  return restore_return(status);
}

int rmq_fault_corrupt_repair(rmq_engine* e, uint32_t dst, int64_t at) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  if (!e->repl || dst >= e->repl->world || dst == e->repl->rank) return RMQ_EINVAL;
  e->rr.flip[dst] = true;
  e->rr.flip_at[dst] = at;
  return RMQ_OK;
}

}  // extern "C"
