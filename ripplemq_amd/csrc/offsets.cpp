// offsets.cpp — consumer-offset commits and their tickets (rmq_commit_consumer_offset, the offsets
// half of rmq_poll_commit) and followers' acks given by hand (rmq_ack).
#include "engine_internal.hpp"

using namespace rmq;

namespace rmq {

namespace {

// The four sections of a commit slot of `cap` items, the same in its pinned block and its device
// copy: partition and consumer (u32), offset and row version (u64).
struct CommitSections {
  uint32_t *pidx, *consumer;
  uint64_t *offset, *ver;
  CommitSections(uint8_t* base, uint32_t cap)
      : pidx(reinterpret_cast<uint32_t*>(base)), consumer(reinterpret_cast<uint32_t*>(base + 4ull * cap)),
        offset(reinterpret_cast<uint64_t*>(base + 8ull * cap)), ver(reinterpret_cast<uint64_t*>(base + 16ull * cap)) {}
  static constexpr uint64_t kItemBytes = 24;
};

// A new generation of a stamp table of `size` words: an entry equal to the generation was seen in
// this call. A fresh table, or a wrapped generation (stale stamps could alias it), starts from zeroes.
uint32_t next_generation(std::vector<uint32_t>& stamp, uint32_t& gen, size_t size) {
  if (stamp.size() != size) {
    stamp.assign(size, 0u);
    gen = 0;
  }
  if (++gen == 0) {
    std::fill(stamp.begin(), stamp.end(), 0u);
    gen = 1;
  }
  return gen;
}

// The next commit slot, its last use complete, with room for n items.
int commit_slot(rmq_engine* e, uint32_t n, rmq_engine::CommitSlot** out) {
  rmq_engine::CommitSlot& cs = e->cslot[e->cslot_next];
  e->cslot_next = (e->cslot_next + 1) % rmq_engine::kCommitSlots;
  if (cs.used) {
    const int rc = event_wait(cs.ev);
    if (rc) return rc;
  }
  cs.used = false;
  if (n > cs.cap) {
    if (cs.h) hipHostFree(cs.h);
    if (cs.d) hipFree(cs.d);
    cs.h = cs.d = nullptr;
    cs.cap = 0;
    const uint32_t cap = std::max<uint32_t>(n, 4096);
    HIP_TRY(hipHostMalloc((void**)&cs.h, CommitSections::kItemBytes * cap, 0));
    int rc = dalloc(&cs.d, CommitSections::kItemBytes * cap);
    if (rc) return rc;
    if (!cs.ev) HIP_TRY(hipEventCreateWithFlags(&cs.ev, hipEventDisableTiming));
    cs.cap = cap;
  }
  *out = &cs;
  return RMQ_OK;
}

// ONE pass from the last item back, straight into the staging slot: the per-item checks, last
// writer wins (PartitionStateMachine.java:71-77: only the last item per (partition, consumer) is
// kept, so the device scatter has no two writers to one slot; a generation stamp per slot instead
// of a hash set), and the new row version of every partition the call commits to (one per call)
// with the ticket's (partition, version) pairs in tv. The kept items end up at [k, n) in call order;
// returns k, and in *rc_all the first failing item's status in call order.
uint32_t fill_commit_slot(rmq_engine* e, const CommitSections& h, const uint32_t* pidx, const uint32_t* consumer,
                          const uint64_t* offset, uint32_t n, int32_t* status,
                          std::vector<std::pair<uint32_t, uint64_t>>& tv, int* rc_all) {
  const uint32_t P = e->cfg.num_partitions, C = e->cfg.max_consumers;
  const uint32_t gen = next_generation(e->lww_stamp, e->lww_gen, (size_t)P * C);
  const uint32_t cgen = next_generation(e->cstamp, e->cstamp_gen, P);
  uint32_t k = n;
  for (uint32_t i = n; i-- > 0;) {
    const uint32_t p = pidx[i], c = consumer[i];
    int st = RMQ_OK;
    if (p >= P)
      st = RMQ_ENOPART;
    else if (!e->is_leader[p])
      st = RMQ_ENOTLEADER;
    else if (c >= C)
      st = RMQ_EINVAL;
    if (status) status[i] = st;
    if (st) {
      *rc_all = st;  // scanning back, the last one set is the first failing item in call order
      continue;
    }
    uint32_t& sl = e->lww_stamp[(size_t)p * C + c];
    if (sl == gen) continue;  // a later item of the call wins
    sl = gen;
    if (e->cstamp[p] != cgen) {  // the partition's first kept item
      e->cstamp[p] = cgen;
      tv.emplace_back(p, ++e->cver[p]);
    }
    --k;
    h.pidx[k] = p;
    h.consumer[k] = c;
    h.offset[k] = offset[i];
    h.ver[k] = e->cver[p];
  }
  return k;
}

int ensure_ctl(rmq_engine* e, uint32_t n) {
  if (n <= e->ctl_cap) return RMQ_OK;
  hipFree(e->d_ctl32);
  hipFree(e->d_ctl64);
  e->ctl_cap = 0;
  uint32_t cap = std::max<uint32_t>(n, 1024);
  int rc = dalloc(&e->d_ctl32, (size_t)cap * 2);
  if (rc) return rc;
  rc = dalloc(&e->d_ctl64, (size_t)cap);
  if (rc) return rc;
  e->ctl_cap = cap;
  return RMQ_OK;
}

}  // namespace

// A consumer-offset ticket (RMQ_TICKET_OFFSETS): are its partitions' rows on a quorum?
int poll_offsets(rmq_engine* e, uint64_t ticket) {
  auto it = std::find_if(e->off_tickets.begin(), e->off_tickets.end(),
                         [ticket](const auto& x) { return x.first == ticket; });
  if (it == e->off_tickets.end()) return RMQ_EINVAL;  // unknown, or resolved already
  int rc = quiesce(e);  // the commit kernels and the ack folds issued so far (no flush)
  if (rc) return rc;
  const size_t P = e->cfg.num_partitions;
  std::vector<uint64_t> cq(P);
  HIP_TRY(hipMemcpy(cq.data(), e->st.cq, P * 8, hipMemcpyDeviceToHost));
  bool done = true, lost = false;
  for (const auto& pv : it->second) {
    if (cq[pv.first] >= pv.second) continue;
    done = false;
    if (!e->is_leader[pv.first]) lost = true;  // leadership moved before its row reached a quorum
  }
  if (!done && !lost) return RMQ_PENDING;
  e->off_tickets.erase(it);
  return done ? RMQ_OK : RMQ_ENOTLEADER;
}

void offsets_free(rmq_engine* e) {
  for (auto& cs : e->cslot) {  // (hipFree and hipHostFree take null)
    hipHostFree(cs.h), hipFree(cs.d);
    if (cs.ev) hipEventDestroy(cs.ev);
    cs = rmq_engine::CommitSlot{};
  }
  hipFree(e->d_ctl32), hipFree(e->d_ctl64);
  e->d_ctl32 = nullptr, e->d_ctl64 = nullptr, e->ctl_cap = 0;
}

}  // namespace rmq

extern "C" {

int rmq_commit_consumer_offset(rmq_engine* e, const uint32_t* pidx, const uint32_t* consumer,
                               const uint64_t* offset, uint32_t n, int32_t* status, uint64_t* ticket) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  if (ticket) *ticket = 0;
  if (!n) return RMQ_OK;
  if (!pidx || !consumer || !offset) return RMQ_EINVAL;
  HIP_TRY(hipSetDevice(e->device));
  // no flush and no wait for the pipeline (it never reads the table): the items go to the device
  // with one copy on the pipeline stream, behind the launches issued so far, from a staging slot
  // whose previous use has completed; a fetch or read-back issued later sees them
  rmq_engine::CommitSlot* slot = nullptr;
  int rc = commit_slot(e, n, &slot);
  if (rc) return rc;
  rmq_engine::CommitSlot& cs = *slot;
  std::vector<std::pair<uint32_t, uint64_t>> tv;
  int rc_all = RMQ_OK;
  const uint32_t k = fill_commit_slot(e, CommitSections(cs.h, cs.cap), pidx, consumer, offset, n, status, tv, &rc_all);
  const uint32_t m = n - k;
  if (!m) return rc_all;
  HIP_TRY(hipMemcpyAsync(cs.d, cs.h, CommitSections::kItemBytes * cs.cap, hipMemcpyHostToDevice, e->main_s));
  const CommitSections d(cs.d, cs.cap);
  ConsumerCommitArgs a{};
  a.st = e->st;
  a.pidx = d.pidx + k;
  a.consumer = d.consumer + k;
  a.offset = d.offset + k;
  a.ver = d.ver + k;
  a.n = m;
  launch_consumer_commit(a, e->main_s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(cs.ev, e->main_s));
  cs.used = true;
  if (ticket) {
    *ticket = RMQ_TICKET_OFFSETS | ++e->off_ticket_seq;
    e->off_tickets.emplace_back(*ticket, std::move(tv));
    while (e->off_tickets.size() > rmq_engine::kMaxOffsetTickets) e->off_tickets.pop_front();  // never polled
  }
  rc = check_err(e);
  return rc ? rc : rc_all;
}

int rmq_ack(rmq_engine* e, const uint32_t* pidx, const uint32_t* slot, const uint64_t* match, uint32_t n) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  if (!n) return RMQ_OK;
  if (!pidx || !slot || !match) return RMQ_EINVAL;
  for (uint32_t i = 0; i < n; ++i) {
    if (pidx[i] >= e->cfg.num_partitions) return RMQ_ENOPART;
    if (slot[i] >= e->cfg.replication_factor) return RMQ_EINVAL;
  }
  int rc = begin_call(e, drain);
  if (rc) return rc;
  rc = ensure_ctl(e, n);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(e->d_ctl32, pidx, n * 4ull, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d_ctl32 + e->ctl_cap, slot, n * 4ull, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d_ctl64, match, n * 8ull, hipMemcpyHostToDevice));
  AckArgs a{};
  a.st = e->st;
  a.pidx = e->d_ctl32;
  a.slot = e->d_ctl32 + e->ctl_cap;
  a.match = e->d_ctl64;
  a.n = n;
  launch_ack(a, e->main_s);
  HIP_TRY(hipGetLastError());
  return drain(e);
}

}  // extern "C"
