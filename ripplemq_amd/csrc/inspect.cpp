// inspect.cpp — the read-backs and the fault injection of the C-ABI: rmq_get_partition_state(s),
// rmq_read_segment, rmq_read_index, rmq_read_consumer_offsets / _table, rmq_replication_stats,
// rmq_read_outbox and the rmq_fault_* hooks of the tests.
//
// None of them flushes: a read waits for what is issued (quiesce, which also runs the late retention
// of the last applied group) and copies; a flip of stored bytes drains first. The single-partition
// reads are the n = 1 case of the range reads.
#include "engine_internal.hpp"

using namespace rmq;

namespace {

// The words of a partition that state_gather_kernel (control.hip) gathers, in its order; the match
// rows follow them. The only place on the host that knows this order.
enum StateWord { kLeo, kUsed, kStartOff, kStartPos, kCommit, kHw, kTerm, kTermStart, kLcommit, kLterm, kHeard,
                 kStateWords };
static_assert(kStateWords == 11, "state_gather_kernel's fields");

// One rmq_partition_state from the gathered words of partition p (field f at v[f * stride]), its
// match row and the host mirrors. Zeroed first, padding included: callers compare the bytes.
void fill_state(const rmq_engine* e, uint32_t p, const uint64_t* v, size_t stride, const uint64_t* match,
                rmq_partition_state* o) {
  const uint32_t RF = e->cfg.replication_factor;
  std::memset(o, 0, sizeof *o);
  o->log_end_offset = v[kLeo * stride];
  o->log_end_pos = v[kUsed * stride];
  o->log_start_offset = v[kStartOff * stride];
  o->log_start_pos = v[kStartPos * stride];
  o->commit = v[kCommit * stride];
  o->high_watermark = v[kHw * stride];
  o->term = v[kTerm * stride];
  o->term_start = v[kTermStart * stride];
  std::copy_n(match, RF, o->match);
  std::copy_n(&e->ranks[(size_t)p * RF], RF, o->replica_rank);
  o->leader_slot = e->leader_slot[p];
  o->is_leader = e->is_leader[p];
  o->segment_bytes = ring_bytes(e->ring[p]);
  o->leader_commit = o->is_leader ? o->commit : v[kLcommit * stride];  // a leader's own commit
  const uint64_t lterm = v[kLterm * stride];
  o->last_log_term = (lterm & kLtermBound) ? 0ull : lterm;  // unknown: a candidate claims none
  o->heard_round = v[kHeard * stride];
  o->voted_term = e->vterm[p];
  o->voted_for = e->vfor[p];
  o->led = e->vled[p];
}

// The states of partitions [first, first + n), n > 0 (engine locked, range checked): every field
// gathered by one kernel into a page-locked staging area, one wait (12 synchronous copies into
// pageable vectors took 0.86 ms for 4,096 partitions).
int read_states(rmq_engine* e, uint32_t first, uint32_t n, rmq_partition_state* o) {
  int rc = begin_call(e, quiesce);
  if (rc) return rc;
  const uint32_t RF = e->cfg.replication_factor;
  const size_t words = (size_t)e->cfg.num_partitions * (kStateWords + RF);
  if (e->state_stage_words < words) {
    if (e->state_stage) hipHostFree(e->state_stage);
    e->state_stage = nullptr;
    e->state_stage_words = 0;
    HIP_TRY(hipHostMalloc((void**)&e->state_stage, words * 8, 0));
    e->state_stage_words = words;
  }
  uint64_t* const v = e->state_stage;
  launch_state_gather(e->st, v, first, n, RF, e->main_s);  // (page-locked: the kernel writes it in place)
  HIP_TRY(hipGetLastError());
  rc = stream_wait(e->main_s);
  for (uint32_t i = 0; i < n && !rc; ++i)
    fill_state(e, first + i, v + i, n, v + (size_t)n * kStateWords + (size_t)i * RF, &o[i]);
  return rc;
}

// The consumer-offset rows of partitions [first, first + n), n > 0 (engine locked, range checked).
int read_consumer_rows(rmq_engine* e, uint32_t first, uint32_t n, uint64_t* out) {
  const int rc = begin_call(e, quiesce);
  const size_t C = e->cfg.max_consumers;
  return rc ? rc : read_words(out, e->st.cons + (size_t)first * C, (size_t)n * C);
}

// XOR a value into stored bytes at a device address, after everything submitted is applied.
template <typename T>
int xor_at(rmq_engine* e, T* at, T mask) {
  T v = 0;
  int rc = begin_call(e, drain);
  if (!rc) rc = read_words(&v, at);
  v ^= mask;
  return rc ? rc : write_words(at, &v);
}

}  // namespace

extern "C" {

int rmq_get_partition_state(rmq_engine* e, uint32_t p, rmq_partition_state* o) {
  if (!e || !o) return RMQ_EINVAL;
  EngineLock g(e);
  if (p >= e->cfg.num_partitions) return RMQ_ENOPART;
  return read_states(e, p, 1, o);
}

int rmq_get_partition_states(rmq_engine* e, uint32_t first, uint32_t n, rmq_partition_state* o) {
  if (!e || (n && !o)) return RMQ_EINVAL;
  EngineLock g(e);
  const uint32_t P = e->cfg.num_partitions;
  if (first > P || n > P - first) return RMQ_ENOPART;
  return n ? read_states(e, first, n, o) : RMQ_OK;
}

int rmq_read_segment(rmq_engine* e, uint32_t replica, uint32_t p, uint64_t ring_off, uint64_t len, uint8_t* out) {
  if (!e || (len && !out)) return RMQ_EINVAL;
  EngineLock g(e);
  if (p >= e->cfg.num_partitions) return RMQ_ENOPART;
  const RingRef rg = ring_of(e, p);
  if (replica >= e->cfg.replication_factor || ring_off > rg.seg || len > rg.seg - ring_off) return RMQ_EINVAL;
  int rc = begin_call(e, quiesce);
  if (!rc && len) rc = read_words(out, e->st.logs + (uint64_t)replica * e->st.rstride + rg.base + ring_off, len);
  return rc;
}

int rmq_read_index(rmq_engine* e, uint32_t p, uint64_t m_first, uint64_t count, uint64_t* out) {
  if (!e || (count && !out)) return RMQ_EINVAL;
  EngineLock g(e);
  if (p >= e->cfg.num_partitions) return RMQ_ENOPART;
  const RingRef rg = ring_of(e, p);
  if (count > rg.icap) return RMQ_EINVAL;
  int rc = begin_call(e, quiesce);
  std::vector<uint64_t> ring((size_t)rg.icap * 2);
  if (!rc) rc = read_words(ring, e->st.index + rg.ibase * 2);
  for (uint64_t k = 0; k < count && !rc; ++k) std::copy_n(&ring[2 * ((m_first + k) % rg.icap)], 2, out + 2 * k);
  return rc;
}

int rmq_read_consumer_offsets(rmq_engine* e, uint32_t p, uint64_t* out) {
  if (!e || !out) return RMQ_EINVAL;
  EngineLock g(e);
  if (p >= e->cfg.num_partitions) return RMQ_ENOPART;
  return read_consumer_rows(e, p, 1, out);
}

int rmq_read_consumer_table(rmq_engine* e, uint32_t first, uint32_t n, uint64_t* out) {
  if (!e || (n && !out)) return RMQ_EINVAL;
  EngineLock g(e);
  if (first > e->cfg.num_partitions || n > e->cfg.num_partitions - first) return RMQ_ENOPART;
  return n ? read_consumer_rows(e, first, n, out) : RMQ_OK;
}

int rmq_fault_flip_ring(rmq_engine* e, uint32_t replica, uint32_t p, uint64_t ring_off, uint32_t xor_mask) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  if (p >= e->cfg.num_partitions) return RMQ_ENOPART;
  const RingRef rg = ring_of(e, p);
  if (replica >= e->cfg.replication_factor || !(local_slots(e, p) >> replica & 1u) || ring_off >= rg.seg ||
      !(xor_mask & 0xFFu))
    return RMQ_EINVAL;
  // one byte inside the partition's own ring block of a local replica region
  return xor_at(e, e->st.logs + (uint64_t)replica * e->st.rstride + rg.base + ring_off, (uint8_t)(xor_mask & 0xFFu));
}

int rmq_fault_flip_index(rmq_engine* e, uint32_t pidx, uint64_t m, uint32_t word, uint64_t xor_mask) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  if (pidx >= e->cfg.num_partitions) return RMQ_ENOPART;
  if (word > 1u || !xor_mask) return RMQ_EINVAL;
  const RingRef rg = ring_of(e, pidx);
  // one word of the partition's own index ring
  return xor_at(e, e->st.index + (rg.ibase + m % rg.icap) * 2 + word, xor_mask);
}

int rmq_replication_stats(rmq_engine* e, rmq_repl_stats* out) {
  if (!e || !out) return RMQ_EINVAL;
  EngineLock g(e);
  std::memset(out, 0, sizeof *out);
  if (!e->repl) return RMQ_OK;
  const Replication* r = e->repl;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(r->xchg_s));
  uint64_t c[7];
  int rc = read_words(c, r->d_counters, 7);
  if (rc) return rc;
  out->world = r->world;
  out->rank = r->rank;
  out->out_entries = (uint32_t)r->lists.xo_p.size();
  out->in_entries = (uint32_t)r->lists.xi_p.size();
  out->rounds = r->rounds;
  out->bytes_sent = r->bytes_sent;
  out->bytes_received = r->bytes_recv;
  out->records_ingested = c[0];
  out->refused_crc = c[1];
  out->refused_log = c[2];
  out->bytes_ingested = c[3];
  out->catchup_entries = c[4];
  out->detached_plans = c[5];
  out->general_plans = c[6];
  out->host_waits = r->host_waits;
  out->host_wait_ns = r->host_wait_ns;
  return RMQ_OK;
}

int rmq_read_outbox(rmq_engine* e, uint32_t dst, uint8_t* out, uint64_t cap, uint64_t* size) {
  if (!e || !size) return RMQ_EINVAL;
  EngineLock g(e);
  *size = 0;
  Replication* r = e->repl;
  if (!r || dst >= r->world) return RMQ_EINVAL;
  if (r->last_set == ~0u) return RMQ_OK;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(r->xchg_s));
  const XchgSet& x = r->sets[r->last_set];
  const uint64_t n = dst == r->rank ? 0 : x.h_sizes[2 * dst];
  *size = n;
  if (!out) return RMQ_OK;
  if (n > cap) return RMQ_ENOSPC;
  return n ? read_words(out, x.outbox + (uint64_t)dst * r->dcap, n) : RMQ_OK;  // region d at d * dcap of the outbox
}

int rmq_fault_drop_rounds(rmq_engine* e, uint32_t n) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  if (!e->repl) return RMQ_EINVAL;
  e->repl->drop_from = e->last_ticket + 1;
  e->repl->drop_n = n;
  return RMQ_OK;
}

int rmq_fault_isolate(rmq_engine* e, uint32_t dst, uint32_t n) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  if (!e->repl || dst >= e->repl->world || dst == e->repl->rank) return RMQ_EINVAL;
  e->repl->iso_from[dst] = e->last_ticket + 1;
  e->repl->iso_n[dst] = n;
  return RMQ_OK;
}

int rmq_fault_cut(rmq_engine* e, uint32_t dst, uint32_t n) {
  int rc = rmq_fault_isolate(e, dst, n);
  if (rc) return rc;
  EngineLock g(e);
  e->repl->cut_notice |= 1u << dst;
  return RMQ_OK;
}

int rmq_fault_corrupt(rmq_engine* e, uint32_t dst, int64_t at) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  if (!e->repl || dst >= e->repl->world || dst == e->repl->rank) return RMQ_EINVAL;
  e->repl->flip[dst] = true;
  e->repl->flip_at[dst] = at;
  return RMQ_OK;
}

}  // extern "C"
