// replication.cpp — replica-log rounds between engines over a Transport (FORMAT.md §9).
//
// Reference: each partition is a jraft group whose leader replicates its log to RF-1 followers
// with AppendEntries and commits on a quorum of acks (BallotBox) — configured in
// PartitionRaftServer.java:82-93 (peers of the group), started by node.apply at
// MessageAppendRequestProcessor.java:59; replicas are spread over brokers by
// PartitionAssigner.java:25-94. Here one engine per GPU leads some partitions and follows others
// (rmq_set_placement); every launch group of appends is one round:
//
//   launch k+1 (stage 2 of group g): the last stage-2 workgroup plans g's outbox (pipeline.hip);
//       after it, the exchange stream swaps {region bytes, records} with every peer;
//   launch k+2 (stage 3 of g): records also go, once per remote slot, into g's outbox;
//   after launch k+3 is issued: the host reads g's sizes (exchanged one launch earlier) and posts
//       on the exchange stream, behind launch k+2: the grouped send/recv of the regions, the
//       follower ingest (CRC32C check, ring + index writes, log end, retention; replicate.hip) and
//       the grouped send/recv of the acks (follower log ends);
//   launch k+5 (three launches after g's stage 3): waits for g's exchange and applies the acks to
//       the matchIndex rows in its partition threads, then the quorum commit rule; the plan of the
//       group that launch scans reads the same acks for its catch-up verdicts (FORMAT.md §9 v3:
//       a refused entry's next round starts at the follower's log end, the gap re-sent from the
//       leader's ring by the catch-up waves of the stage-3 launch).
//
// Every rank makes the same calls in the same order (rounds are collective, like the launches
// that drive them): with a transport attached, launch groups close only when full, and control
// calls that flush (rmq_sync, placement, leadership) are collective. At a drain the remaining
// rounds are exchanged and their acks applied by a separate kernel.
#include "engine_internal.hpp"

namespace rmq {

namespace {

// A device buffer sized by the placement (zeroed), noted on the record that free_placed frees from,
// also where the zeroing failed.
template <typename T>
int placed_alloc(Replication* r, T** d, size_t count) {
  const int rc = dalloc(d, count);
  if (*d) r->placed.note(d);
  return rc;
}

template <typename T>
int upload(Replication* r, T** d, const std::vector<T>& h) {
  const int rc = placed_alloc(r, d, h.size());
  return rc || h.empty() ? rc : write_words(*d, h);
}

// Every buffer of the placement before this one, the engine's two views of them included.
void free_placed(rmq_engine* e) {
  e->repl->placed.free_all();
  e->st.outidx = nullptr;
  e->st.eackv = nullptr;
}

}  // namespace

// The leader's catch-up state of every out entry starts over (FORMAT.md §9: placement and leader
// start): next = the leader's log end, no request, no catch-up round. Engine drained.
int reset_catchup(rmq_engine* e) {
  Replication* r = e->repl;
  const std::vector<uint32_t>& xo_p = r->lists.xo_p;
  const size_t n = xo_p.size();
  if (!n) return RMQ_OK;
  const uint32_t P = e->cfg.num_partitions;
  std::vector<uint64_t> leo(P), used(P), nx(2 * n);
  HIP_TRY(hipMemcpy(leo.data(), e->st.leo, P * 8ull, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(used.data(), e->st.used, P * 8ull, hipMemcpyDeviceToHost));
  for (size_t k = 0; k < n; ++k) {
    nx[2 * k] = leo[xo_p[k]];
    nx[2 * k + 1] = used[xo_p[k]];
  }
  HIP_TRY(hipMemcpy(r->d_xnext, nx.data(), nx.size() * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(r->d_xreq, 0, n * 32));
  HIP_TRY(hipMemset(r->d_xcu, 0, n * 8));
  return RMQ_OK;
}

namespace {

// The two fixed-size words of every entry, both ways: to peer q those of send's entries for q
// (grouped by sstart), from q those of recv's entries (grouped by rstart).
Exchange entry_swap(const Replication* r, uint64_t* send, const std::vector<uint32_t>& sstart, uint64_t* recv,
                    const std::vector<uint32_t>& rstart) {
  Exchange x;
  for (uint32_t q = 0; q < r->world; ++q) {
    const EntrySpan s = entry_span(sstart, q), g = entry_span(rstart, q);
    x.peer(q, send + s.word, q == r->rank ? 0 : s.bytes, recv + g.word, q == r->rank ? 0 : g.bytes);
  }
  return x;
}

// The follower ingest of the round in set x, laid out as l.
IngestArgs ingest_args(const rmq_engine* e, const XchgSet& x, const RoundLayout& l) {
  const Replication* r = e->repl;
  IngestArgs a{};
  a.st = e->st;
  a.sets[0] = e->sets[0];
  a.sets[1] = e->sets[1];
  a.inbox = x.inbox;
  std::copy_n(l.region, kMaxWorld, a.region);
  std::copy_n(l.rn, kMaxWorld, a.rbytes);
  std::copy_n(l.task0, kMaxWorld + 1, a.task0);
  a.xi_p = r->d_xi_p;
  a.xi_slot = r->d_xi_slot;
  a.xi_start = r->d_xi_start;
  a.world = r->world;
  a.rank = r->rank;
  a.n_in = (uint32_t)r->lists.xi_p.size();
  a.C = e->cfg.max_consumers;
  a.bad = r->d_bad;
  a.acc = r->d_acc;
  a.base = r->d_base;
  a.cdesc = r->d_cdesc;
  a.ackout = x.ackout;
  a.items = r->d_items;
  constexpr uint32_t NW = 1 + kMaxWorld;  // rounds alternate halves of d_nitems
  uint32_t* cur = r->d_nitems + (r->nitems_par ? NW : 0u);
  a.n_items = cur;
  a.insane = cur + 1;
  a.n_items_next = r->d_nitems + (r->nitems_par ? 0u : NW);
  a.keysum_in = r->d_keysum_in;
  a.items_cap = (uint32_t)r->items_cap;
  a.items_grid = l.items;
  a.crc = e->d_crc;
  a.counters = r->d_counters;
  a.stamp = x.round + 1ull;  // (rmq_leader_silent's clock: rounds ingested)
  return a;
}

// The plan of stage 2's group in set x (PipeArgs::xp2; the acks it reads: repl_before_launch).
XPlanArgs xplan_args(const rmq_engine* e, const XchgSet& x) {
  const Replication* r = e->repl;
  XPlanArgs a{};
  a.xo_p = r->d_xo_p;
  a.xo_slot = r->d_xo_slot;
  a.xo_start = r->d_xo_start;
  a.keysum = r->d_keysum;
  a.world = r->world;
  a.rank = r->rank;
  a.n_out = (uint32_t)r->lists.xo_p.size();
  a.C = e->cfg.max_consumers;
  a.count = x.count;
  a.xe = x.xe;
  a.outbox = x.outbox;
  a.sizes = x.sizes;
  a.round = x.round;
  a.reserve = r->reserve;
  a.xnext = r->d_xnext;
  a.xreq = r->d_xreq;
  a.xcu = r->d_xcu;
  a.xdec = r->d_xdec;
  a.xtot = r->d_xtot;
  a.dflag = r->d_dflag;
  // the commit the round carries: the slot of the launch before this one (launch_seq not yet advanced)
  a.csnap = e->st.csnap + (size_t)(e->launch_seq & 1ull) * e->cfg.num_partitions;
  a.dirty = e->st.cdirty;
  a.rowv = x.rowv;
  a.xc = x.xc;
  a.xc_n = x.xc_n;
  a.counters = r->d_counters + 4;
  a.dcap = r->dcap;
  return a;
}

NoticeArgs notice_args(const rmq_engine* e) {
  const Replication* r = e->repl;
  NoticeArgs a{};
  a.st = e->st;
  a.sets[0] = e->sets[0];
  a.sets[1] = e->sets[1];
  a.xo_p = r->d_xo_p;
  a.out = r->d_nout;
  a.xi_p = r->d_xi_p;
  a.in = r->d_nin;
  a.n_out = (uint32_t)r->lists.xo_p.size();
  a.n_in = (uint32_t)r->lists.xi_p.size();
  a.stamp = r->stamp;
  return a;
}

AckApplyArgs ack_apply_args(const rmq_engine* e, const XchgSet& x) {
  AckApplyArgs a{};
  a.st = e->st;
  a.outidx = e->repl->d_outidx;
  a.ackin = x.ackin;
  a.rowv = x.rowv;
  a.xreq = e->repl->d_xreq;
  a.acks_round = x.round;
  return a;
}

// Post the {region bytes, records} swap of the group in set s (after its stage-2 launch). drop: the
// leader sends no region this round; lost: bit q, the region to q is lost (rmq_fault_isolate).
int post_sizes(rmq_engine* e, uint32_t s, bool drop, uint32_t lost) {
  Replication* r = e->repl;
  XchgSet& x = r->sets[s];
  const uint32_t W = r->world;
  HIP_TRY(hipStreamWaitEvent(r->xchg_s, x.ev_s2, 0));
  if (drop) HIP_TRY(hipMemsetAsync(x.sizes, 0, 2ull * W * 8, r->xchg_s));  // no region to anyone
  for (uint32_t q = 0; q < W && !drop; ++q)
    if ((lost >> q) & 1u) HIP_TRY(hipMemsetAsync(x.sizes + 2 * q, 0, 16, r->xchg_s));
  int rc = fixed_swap(r, x.sizes, x.sizes + 2 * W, 2, 16).post(r);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(x.h_sizes, x.sizes, 4ull * W * 8, hipMemcpyDeviceToHost, r->xchg_s));
  HIP_TRY(hipEventRecord(x.ev_sz, r->xchg_s));
  return RMQ_OK;
}

// Post the round of the group in set s (applied already): regions, follower ingest, acks.
int post_round(rmq_engine* e, uint32_t s) {
  Replication* r = e->repl;
  XchgSet& x = r->sets[s];
  const uint32_t W = r->world, me = r->rank;
  // RCCL's grouped send/recv take host-side byte counts: the sizes were swapped one launch earlier,
  // so this normally finds them landed; a wait is counted (rmq_repl_stats.host_waits)
  if (hipEventQuery(x.ev_sz) == hipErrorNotReady) {
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = event_wait(x.ev_sz);
    if (rc) return rc;
    r->host_waits++;
    r->host_wait_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  }
  const RoundLayout l = plan_round(x.h_sizes, W, me, r->dcap, verify_records_per_task(), r->items_cap,
                                   r->lists.xi_p.size(), kCopyChunk);
  if (l.smax > r->dcap || l.ro > r->in_cap) {
    std::fprintf(stderr, "ripplemq: replication round exceeds its buffers (%llu/%llu out, %llu/%llu in)\n",
                 (unsigned long long)l.smax, (unsigned long long)r->dcap, (unsigned long long)l.ro,
                 (unsigned long long)r->in_cap);
    return RMQ_EDEVICE;
  }
  Exchange regions;
  for (uint32_t q = 0; q < W; ++q) regions.peer(q, x.outbox + l.soff[q], l.sn[q], x.inbox + l.region[q], l.rn[q]);
  HIP_TRY(hipStreamWaitEvent(r->xchg_s, x.ev_s3, 0));
  for (uint32_t q = 0; q < W; ++q)  // rmq_fault_corrupt
    if (r->flip[q] && l.sn[q]) {
      launch_flip(static_cast<uint8_t*>(regions.sb[q]), l.sn[q], r->flip_at[q], r->xchg_s);
      r->flip[q] = false;
    }
  int rc = regions.post(r);
  if (rc) return rc;
  const IngestArgs a = ingest_args(e, x, l);
  if (a.stamp > r->stamp) r->stamp = a.stamp;
  r->stamp_time[a.stamp % 64] = std::chrono::steady_clock::now();
  launch_ingest(a, l.tasks, l.items, e->knob.verify_wgs, r->xchg_s);
  if (a.n_in) r->nitems_par ^= 1u;  // (prepare ran: it cleared the other half)
  HIP_TRY(hipGetLastError());
  // acks: {log end | status, position} of every in entry back to its leader, fixed sizes both ways
  rc = entry_swap(r, x.ackout, r->lists.xi_start, x.ackin, r->lists.xo_start).post(r);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(x.ev_x, r->xchg_s));
  r->rounds++;
  for (uint32_t q = 0; q < W; ++q) r->bytes_sent += l.sn[q];
  r->bytes_recv += l.ro;
  r->last_set = s;
  r->acking.push_back(s);
  return RMQ_OK;
}

}  // namespace

int repl_attach(rmq_engine* e, Transport* t) {
  if (e->repl) return RMQ_EINVAL;
  if (t->world() > kMaxWorld || t->rank() != e->cfg.rank || t->world() <= e->cfg.rank) return RMQ_EINVAL;
  // groups must close by count alone so every rank forms the same rounds
  if (e->group_max * e->max_tiles > kMaxTiles) return RMQ_EINVAL;
  Replication* r = new (std::nothrow) Replication();
  if (!r) return RMQ_ENOMEM;
  r->xport = t;
  r->world = t->world();
  r->rank = t->rank();
  e->repl = r;
  HIP_TRY(hipStreamCreateWithFlags(&r->xchg_s, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&r->ev_notice, hipEventDisableTiming));
  for (XchgSet& x : r->sets) {
    HIP_TRY(hipEventCreateWithFlags(&x.ev_s2, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&x.ev_s3, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&x.ev_sz, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&x.ev_x, hipEventDisableTiming));
    int rc = dalloc(&x.count, 1);
    if (rc) return rc;
    HIP_TRY(hipHostMalloc((void**)&x.h_sizes, 4ull * kMaxWorld * 8, 0));
  }
  int rc = dalloc(&r->d_counters, 7);
  if (!rc) rc = dalloc(&r->d_lastg, e->cfg.num_partitions);
  if (!rc) rc = dalloc(&r->d_shake, 8ull * kMaxWorld);
  if (!rc && !e->st.csnap) rc = owned_dalloc(e, &e->st.csnap, 2ull * e->cfg.num_partitions);
  if (rc) return rc;
  {
    // both slots start at the current commits (the first plan reads the slot of the launch before)
    for (uint32_t k = 0; k < 2; ++k)
      HIP_TRY(hipMemcpy(e->st.csnap + (size_t)k * e->cfg.num_partitions, e->st.commit,
                        e->cfg.num_partitions * 8ull, hipMemcpyDeviceToDevice));
  }
  return repl_set_lists(e);
}

void repl_free(rmq_engine* e) {
  Replication* r = e->repl;
  if (!r) return;
  if (r->xchg_s) hipStreamSynchronize(r->xchg_s);
  free_placed(e);
  // what repl_attach made
  for (XchgSet& x : r->sets) {
    hipEvent_t evs[] = {x.ev_s2, x.ev_s3, x.ev_sz, x.ev_x};
    for (hipEvent_t v : evs)
      if (v) hipEventDestroy(v);
    if (x.count) hipFree(x.count);
    if (x.h_sizes) hipHostFree(x.h_sizes);
  }
  if (r->d_counters) hipFree(r->d_counters);
  if (r->d_lastg) hipFree(r->d_lastg);
  if (r->d_shake) hipFree(r->d_shake);
  if (r->ev_notice) hipEventDestroy(r->ev_notice);
  if (r->xchg_s) hipStreamDestroy(r->xchg_s);
  delete r->xport;
  delete r;
  e->repl = nullptr;
}

namespace {

// Step 1 of repl_set_lists: the out / in lists of the engine's placement, into the host mirrors.
void plan_placement(rmq_engine* e) {
  Placement pl;
  pl.P = e->cfg.num_partitions, pl.RF = e->cfg.replication_factor, pl.W = e->repl->world, pl.me = e->repl->rank;
  pl.ranks = e->ranks.data(), pl.leader_slot = e->leader_slot.data(), pl.key = e->key.data();
  e->repl->lists = plan_lists(pl, kMaxRemote, RMQ_MAX_RF);
}

// Step 2, the handshake: what I send to q must be what q expects from me, and every rank learns
// whether all pairs agree (two exchanges, so no rank starts rounds that another refuses).
int handshake(Replication* r) {
  const ReplLists& l = r->lists;
  const uint32_t W = r->world, me = r->rank;
  uint64_t* d = r->d_shake;
  std::vector<uint64_t> h(8ull * W, 0);  // [q]: send {entries, keysum}; [W + q]: recv; [2W..] verdicts
  for (uint32_t q = 0; q < W; ++q) {
    h[2 * q] = l.xo_start[q + 1] - l.xo_start[q];
    h[2 * q + 1] = l.keysum[q];
  }
  int rc = write_words(d, h);
  if (!rc) rc = fixed_swap(r, d, d + 2 * W, 2, 16).post(r);
  if (!rc) rc = hip_fail(hipStreamSynchronize(r->xchg_s));
  if (!rc) rc = read_words(h, d);
  if (rc) return rc;
  uint64_t verdict = l.bad ? 1 : 0;
  for (uint32_t q = 0; q < W; ++q)
    if (q != me && (h[2 * W + 2 * q] != l.xi_start[q + 1] - l.xi_start[q] || h[2 * W + 2 * q + 1] != l.keysum_in[q]))
      verdict = 1;
  for (uint32_t q = 0; q < W; ++q) h[4 * W + q] = verdict;
  rc = write_words(d + 4 * W, h.data() + 4 * W, W);
  if (!rc) rc = fixed_swap(r, d + 4 * W, d + 5 * W, 1, 8).post(r);
  if (!rc) rc = hip_fail(hipStreamSynchronize(r->xchg_s));
  if (!rc) rc = read_words(h.data() + 5 * W, d + 5 * W, W);
  if (rc) return rc;
  for (uint32_t q = 0; q < W; ++q) verdict |= q != me ? h[5 * W + q] : 0;
  if (verdict) {
    std::fprintf(stderr, "ripplemq: replica placement differs between ranks (rank %u)\n", me);
    return RMQ_EINVAL;
  }
  return RMQ_OK;
}

// The FORMAT.md §9 bounds of the placement's round buffers.
ReplBounds placement_bounds(const rmq_engine* e) {
  const ReplLists& l = e->repl->lists;
  BoundsShape s;
  s.group_max = e->group_max, s.max_batch_records = e->cfg.max_batch_records;
  s.max_batch_bytes = e->cfg.max_batch_bytes, s.max_consumers = e->cfg.max_consumers;
  s.W = e->repl->world, s.RF = e->cfg.replication_factor, s.max_remote = l.max_remote;
  s.n_out = l.xo_p.size(), s.n_in = l.xi_p.size();
  return plan_bounds(s, {kRegionHdr, kDirEntry, kCopyChunk});
}

// Step 3: the lists on the device and the per-entry state, zeroed.
int upload_lists(Replication* r, const ReplBounds& b) {
  const ReplLists& l = r->lists;
  int rc = upload(r, &r->d_xo_p, l.xo_p);
  if (!rc) rc = upload(r, &r->d_xo_slot, l.xo_slot);
  if (!rc) rc = upload(r, &r->d_xo_start, l.xo_start);
  if (!rc) rc = upload(r, &r->d_keysum, l.keysum);
  if (!rc) rc = upload(r, &r->d_keysum_in, l.keysum_in);
  if (!rc) rc = upload(r, &r->d_outidx, l.outidx);
  if (!rc) rc = upload(r, &r->d_xi_p, l.xi_p);
  if (!rc) rc = upload(r, &r->d_xi_slot, l.xi_slot);
  if (!rc) rc = upload(r, &r->d_xi_start, l.xi_start);
  if (!rc) rc = placed_alloc(r, &r->d_bad, b.n_in);
  if (!rc) rc = placed_alloc(r, &r->d_acc, b.n_in);
  if (!rc) rc = placed_alloc(r, &r->d_base, 2 * b.n_in);
  if (!rc) rc = placed_alloc(r, &r->d_cdesc, 4 * b.n_in);
  if (!rc) rc = placed_alloc(r, &r->d_xnext, 2 * b.n_out);
  if (!rc) rc = placed_alloc(r, &r->d_xreq, 4 * b.n_out);
  if (!rc) rc = placed_alloc(r, &r->d_xcu, b.n_out);
  if (!rc) rc = placed_alloc(r, &r->d_dflag, r->world);
  if (!rc) rc = placed_alloc(r, &r->d_nout, 2 * b.n_out);
  if (!rc) rc = placed_alloc(r, &r->d_nin, 2 * b.n_in);
  if (!rc) rc = placed_alloc(r, &r->d_xdec, b.n_out);
  if (!rc) rc = placed_alloc(r, &r->d_xtot, b.n_out);
  return rc;
}

// Step 4: the bounds post_round answers RMQ_EDEVICE against, the copy items and every set's buffers.
int alloc_round_buffers(Replication* r, const ReplBounds& b) {
  r->reserve = b.reserve;
  r->dcap = b.dcap;
  r->out_cap = b.out_cap;
  r->in_cap = b.in_cap;
  r->items_cap = b.items_cap;
  int rc = placed_alloc(r, &r->d_items, 2 * b.items_cap);
  if (!rc) rc = placed_alloc(r, &r->d_nitems, 2 * (1 + kMaxWorld));  // both halves zero
  r->nitems_par = 0;
  for (XchgSet& x : r->sets) {
    if (!rc) rc = placed_alloc(r, &x.outbox, b.out_cap);
    if (!rc) rc = placed_alloc(r, &x.inbox, b.in_cap);
    if (!rc) rc = placed_alloc(r, &x.xe, b.n_out);
    if (!rc) rc = placed_alloc(r, &x.xc, b.n_out);
    if (!rc) rc = placed_alloc(r, &x.xc_n, 2);
    if (!rc) rc = placed_alloc(r, &x.sizes, 4ull * r->world);
    if (!rc) rc = placed_alloc(r, &x.ackout, 2 * b.n_in);
    if (!rc) rc = placed_alloc(r, &x.ackin, 2 * b.n_out);
    if (!rc) rc = placed_alloc(r, &x.rowv, b.n_out);
  }
  return rc;
}

// Step 5, the consumer-offset rows: the followers acknowledge them afresh under the new lists (the
// rows of every led partition with committed offsets go out with the next round) and every
// partition's row quorum is recomputed (pending offset tickets wait for those rounds' acks).
int rearm_consumer_rows(rmq_engine* e, const ReplBounds& b) {
  Replication* r = e->repl;
  const uint32_t P = e->cfg.num_partitions;
  int rc = placed_alloc(r, &r->d_eackv, b.n_out);
  if (rc) return rc;
  e->st.outidx = r->d_outidx;
  e->st.eackv = r->d_eackv;
  std::vector<uint32_t> dirty(P, 0u);
  bool any = false;
  for (uint32_t p = 0; p < P; ++p)
    if (e->is_leader[p] && e->cver[p]) dirty[p] = 1u, any = true;
  if (any) {
    std::vector<uint32_t> cur(P);
    rc = read_words(cur, e->st.cdirty);
    for (uint32_t p = 0; p < P; ++p) dirty[p] |= cur[p];
    if (!rc) rc = write_words(e->st.cdirty, dirty);
    if (rc) return rc;
  }
  launch_row_quorum_all(e->st, e->main_s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->main_s));
  return RMQ_OK;
}

}  // namespace

// Out / in lists from the placement, the collective consistency check, and the round buffers.
// Called with the engine drained, by every rank. A refused handshake leaves the host mirrors
// replaced and every device buffer (with DevState::outidx / eackv) the old placement's.
int repl_set_lists(rmq_engine* e) {
  Replication* r = e->repl;
  plan_placement(e);
  int rc = handshake(r);
  if (rc) return rc;
  free_placed(e);
  const ReplBounds b = placement_bounds(e);
  rc = upload_lists(r, b);
  if (!rc) rc = alloc_round_buffers(r, b);
  if (!rc) rc = rearm_consumer_rows(e, b);
  return rc ? rc : reset_catchup(e);
}

void repl_pipe_args(rmq_engine* e, PipeArgs& a, const GroupFlight* s2, const GroupFlight* s3) {
  Replication* r = e->repl;
  if (!r) return;
  a.lastg = r->d_lastg;               // kept by every launch that applies a group
  // every rank numbers every round (the follower side stamps its ingest with it), also one that
  // leads nothing with a remote replica
  if (s2) r->sets[s2->set].round = r->planned++;
  if (r->lists.xo_p.empty()) return;  // nothing led here has a remote replica
  a.outidx = r->d_outidx;
  if (s2) a.xp2 = xplan_args(e, r->sets[s2->set]);
  if (s3) {
    XchgSet& x = r->sets[s3->set];
    a.xe3 = x.xe;
    a.outbox3 = x.outbox;
    a.xc3 = x.xc;
    a.xc3_n = x.xc_n;
    a.wgc = 2u * e->cu_count / (kPipeThreadsXR / 64u);  // two catch-up waves per CU (most rounds: none)
  }
}

// Before issuing launch launch_seq + 1: the acks of the group applied three launches earlier.
int repl_before_launch(rmq_engine* e, PipeArgs& a) {
  Replication* r = e->repl;
  if (!r || r->acking.empty()) return RMQ_OK;
  const uint32_t s = r->acking.front();
  if (r->sets[s].applied_launch + 3 > e->launch_seq + 1) return RMQ_OK;
  HIP_TRY(hipStreamWaitEvent(e->main_s, r->sets[s].ev_x, 0));
  if (!r->lists.xo_p.empty()) {
    a.ackin = r->sets[s].ackin;
    a.ackrowv = r->sets[s].rowv;
    a.acks_round = r->sets[s].round;
    if (a.xp2.n_out) {  // the plan of this launch turns refusals into catch-up verdicts itself
      a.xp2.ackin = a.ackin;
      a.xp2.acks_round = a.acks_round;
    } else {  // no plan reads these acks: the partition threads keep the requests
      a.xreq = r->d_xreq;
    }
  }
  r->acking.pop_front();
  return RMQ_OK;
}

// After launch launch_seq: post the size swap of its stage-2 group and the rounds of the groups
// applied by earlier launches.
int repl_after_launch(rmq_engine* e, const GroupFlight* s2, const GroupFlight* s3) {
  Replication* r = e->repl;
  if (!r) return RMQ_OK;
  // the rounds of groups applied by earlier launches first: on the exchange stream they then wait
  // only for their own apply launch, not behind the size swap of this launch's group (which waits
  // for this whole launch)
  while (!r->sized.empty() && r->sets[r->sized.front()].applied_launch < e->launch_seq) {
    int rc = post_round(e, r->sized.front());
    if (rc) return rc;
    r->sized.pop_front();
  }
  if (s2) {
    HIP_TRY(hipEventRecord(r->sets[s2->set].ev_s2, e->main_s));
    const bool drop = r->drop_n && s2->b[0].ticket >= r->drop_from;
    if (drop) r->drop_n--;
    uint32_t lost = 0;
    for (uint32_t q = 0; q < r->world; ++q)
      if (r->iso_n[q] && s2->b[0].ticket >= r->iso_from[q]) {
        lost |= 1u << q;
        r->iso_n[q]--;
      }
    int rc = post_sizes(e, s2->set, drop, lost);
    if (rc) return rc;
  }
  if (s3) {
    XchgSet& x = r->sets[s3->set];
    HIP_TRY(hipEventRecord(x.ev_s3, e->main_s));
    x.applied_launch = e->launch_seq;
    r->sized.push_back(s3->set);
  }
  return RMQ_OK;
}

// Commit notices (FORMAT.md §9 v4, the heartbeat of a drain): every leader sends each follower its
// {commit, term} per entry of their list after the drain's acks are in; the followers learn it.
// Collective like the rounds before it (every rank drains the same rounds).
int post_notices(rmq_engine* e) {
  Replication* r = e->repl;
  const std::vector<uint32_t>& xo_start = r->lists.xo_start;
  const NoticeArgs a = notice_args(e);
  launch_notice_fill(a, e->main_s);  // after the acks applied on the pipeline stream
  HIP_TRY(hipGetLastError());
  for (uint32_t q = 0; q < r->world; ++q)  // rmq_fault_cut: these notices are lost (term 0: ignored)
    if (((r->cut_notice >> q) & 1u) && xo_start[q + 1] > xo_start[q])
      HIP_TRY(hipMemsetAsync(r->d_nout + entry_span(xo_start, q).word, 0, entry_span(xo_start, q).bytes, e->main_s));
  r->cut_notice = 0;
  HIP_TRY(hipEventRecord(r->ev_notice, e->main_s));
  HIP_TRY(hipStreamWaitEvent(r->xchg_s, r->ev_notice, 0));
  int rc = entry_swap(r, r->d_nout, xo_start, r->d_nin, r->lists.xi_start).post(r);
  if (rc) return rc;
  launch_notice_apply(a, r->xchg_s);
  HIP_TRY(hipGetLastError());
  // the pipeline stream sees the followers' new commits before anything issued after the drain
  HIP_TRY(hipEventRecord(r->ev_notice, r->xchg_s));
  HIP_TRY(hipStreamWaitEvent(e->main_s, r->ev_notice, 0));
  return RMQ_OK;
}

// After the pipeline is flushed: post the remaining rounds, apply their acks, and (if any round
// was in flight) exchange the commit notices.
int repl_drain(rmq_engine* e) {
  Replication* r = e->repl;
  if (!r) return RMQ_OK;
  const bool rounds = !r->sized.empty() || !r->acking.empty();
  while (!r->sized.empty()) {
    int rc = post_round(e, r->sized.front());
    if (rc) return rc;
    r->sized.pop_front();
  }
  while (!r->acking.empty()) {
    XchgSet& x = r->sets[r->acking.front()];
    HIP_TRY(hipStreamWaitEvent(e->main_s, x.ev_x, 0));
    if (!r->lists.xo_p.empty()) {
      launch_ack_apply(ack_apply_args(e, x), e->main_s);
      HIP_TRY(hipGetLastError());
    }
    r->acking.pop_front();
  }
  if (rounds) {
    int rc = post_notices(e);
    if (rc) return rc;
  }
  HIP_TRY(hipStreamSynchronize(r->xchg_s));
  return RMQ_OK;
}

}  // namespace rmq
