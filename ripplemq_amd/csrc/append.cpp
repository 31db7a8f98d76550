// append.cpp — the append pipeline and its tickets (rmq_append, rmq_poll_commit, rmq_ticket_stats,
// rmq_sync). Appended batches are collected into groups of up to cfg.pipeline_depth; each full group
// issues exactly ONE kernel launch (pipeline.hip) that ranks it (stage 1), scans the group before
// (stage 2), applies the one before that (stage 3) and evaluates the retention of the one before that
// (stage 4). A batch is therefore applied two launches after its group's own; rmq_poll_commit /
// rmq_sync / any control call close the forming group and flush the pipeline with up to three more
// launches that carry only the later stages. No host synchronisation and no HIP events sit on the
// append path: launch k reports launch k-1 complete through a host-visible word, and the tail is read
// with hipStreamQuery. The workgroups of each role of a launch are launch_plan.hpp's plan_roles.
#include "engine_internal.hpp"

using namespace rmq;

namespace rmq {

namespace {

// The groups of one launch: stage 1 on s1, 2 on s2, 3 on s3, 4 on s4 (each may be null).
struct Stages {
  const GroupFlight *s1, *s2, *s3, *s4;
};

PipeGroup make_group(const rmq_engine* e, const GroupFlight& g) {
  PipeGroup G{};
  uint32_t tile = 0, task = 0;
  for (uint32_t j = 0; j < kMaxGroup; ++j) {
    G.tile0[j] = tile;
    G.task0[j] = task;
    if (j < g.nb) {
      const InFlight& f = g.b[j];
      G.b[j] = f.b;
      G.stats[j] = e->d_stats + (size_t)(f.ticket % kStatsRing) * e->max_tasks;
      tile += f.b.tiles;
      task += (f.b.n + kTaskRecs - 1) / kTaskRecs;
    }
  }
  G.tile0[kMaxGroup] = tile;
  G.task0[kMaxGroup] = task;
  G.nb = g.nb;
  G.tiles = tile;
  return G;
}

// The arguments every launch takes from the engine alone.
void pipe_args_common(const rmq_engine* e, PipeArgs& a) {
  a.st = e->st;
  a.cur = e->sets[e->applied & 1u];
  a.nxt = e->sets[(e->applied + 1) & 1u];
  a.key_passes = e->key_passes;
  a.key_bits = e->key_bits;
  a.rank_mode = e->knob.rank_mode;
  a.steal = e->knob.steal;
  a.prio = e->knob.prio;
  a.gt = e->max_group_tiles;
  a.crc = e->d_crc;
  a.done_word = e->done_dev;
  a.ret_late = e->done_dev + 1;
  a.rlate = e->d_rlate;
  a.debug = e->knob.debug;
}

// Each stage's group and scratch set.
int stage_groups(rmq_engine* e, PipeArgs& a, const Stages& g) {
  const auto put = [e](const GroupFlight* s, PipeGroup& group, PipeScratch& scratch) {
    if (s) group = make_group(e, *s), scratch = e->scratch[s->set];
  };
  put(g.s1, a.g1, a.s1);
  put(g.s2, a.g2, a.s2);
  put(g.s3, a.g3, a.s3);
  put(g.s4, a.g4, a.s4);
  if (g.s1) {
    if (e->set_reset & (1u << g.s1->set)) {  // a drain skipped the stage 4 that resets the set's list and sums
      HIP_TRY(hipMemsetAsync(a.s1.bacc, 0, kMaxGroup * 2 * sizeof(uint64_t), e->main_s));
      HIP_TRY(hipMemsetAsync(a.s1.nbig, 0, 4 * sizeof(uint32_t), e->main_s));
      e->set_reset &= ~(1u << g.s1->set);
    }
    a.s1_xcd = e->knob.s1_xcd;
  }
  return RMQ_OK;
}

// The launch as plan_roles sees it, once the replication hooks have set a.outidx and a.ackin: the
// kernel with a transport (outboxes) runs 512-thread workgroups, the single-GPU one 256.
LaunchShape launch_shape(const rmq_engine* e, const PipeArgs& a, const Stages& g) {
  LaunchShape l;
  l.P = e->cfg.num_partitions;
  l.scan_threads = (l.P + kScanCols - 1) / kScanCols * kScanLanes;
  l.cu_count = e->cu_count;
  l.transport = a.outidx != nullptr;
  l.threads = l.transport ? kPipeThreadsXR : kPipeThreads;
  l.wgs_per_cu = pipeline_wgs_per_cu(l.threads);
  l.acks = a.ackin != nullptr;
  l.repl = e->repl != nullptr;
  l.s1 = g.s1, l.s2 = g.s2, l.s3 = g.s3, l.s4 = g.s4;
  l.s1_tiles = g.s1 ? g.s1->tiles : 0u;
  l.s3_tasks = g.s3 ? g.s3->tasks : 0u;
  return l;
}

void set_roles(PipeArgs& a, const RolePlan& r) {
  a.wg1 = r.wg1, a.wg2 = r.wg2, a.wgp = r.wgp, a.wg3 = r.wg3, a.wgb = r.wgb;
  a.s3_lead = r.s3_lead, a.s3_pair = r.s3_pair, a.s3_roles = r.s3_roles, a.s3_xcd = r.s3_xcd;
  a.s3_stage = r.s3_stage;
}

// The launch's number, its phase stamps if it is the stamped one, and the profile region's count;
// returns the event the launch itself records at its start (the region's first launch), else null.
hipEvent_t number_launch(rmq_engine* e, PipeArgs& a, const RolePlan& plan, const GroupFlight* s3) {
  a.launch_seq = ++e->launch_seq;
  e->st.csnap_slot = (uint32_t)(a.launch_seq & 1ull);  // control kernels after this launch write its slot
  if (e->d_stamps && a.launch_seq == e->knob.stamps_at) {
    a.stamps = e->d_stamps;
    e->stamps_plan = plan;
  }
  hipEvent_t ev_start = nullptr;
  rmq_engine::ProfRegion& r = e->region;
  if (e->profile && !r.ended) {
    if (!r.started) {
      ev_start = r.t0;  // recorded by the launch itself (no separate hipEventRecord call)
      r.started = true;
    }
    r.launches++;
    if (s3) r.batches += s3->nb;
  }
  return ev_start;
}

// Two launches side by side: ranking on rank_s, apply on main_s (Knobs::split).
int issue_split(rmq_engine* e, const PipeArgs& a, hipEvent_t ev_start) {
  PipeArgs ra = a, aa = a;
  ra.wgp = ra.wg3 = ra.wgb = ra.wgc = ra.s3_lead = 0;
  ra.done_word = nullptr;
  aa.wg1 = aa.wg2 = 0;
  if (ra.wg1 + ra.wg2) {
    HIP_TRY(hipEventRecord(e->ev_pre_rank, e->main_s));  // apply L - 1 and the control work before it
    HIP_TRY(hipStreamWaitEvent(e->rank_s, e->ev_pre_rank, 0));
    launch_pipeline(ra, e->rank_s, ev_start);
    HIP_TRY(hipGetLastError());
    ev_start = nullptr;
    if (e->knob.split == 2) {  // (timing experiment: the two launches one after the other)
      HIP_TRY(hipEventRecord(e->ev_rank[a.launch_seq & 1u], e->rank_s));
      e->rank_seq = a.launch_seq;
    }
  }
  if (aa.wgp + aa.wg3 + aa.wgb + aa.wgc) {
    if (e->rank_seq) {  // the scans of the group it applies (the last rank launch before this one)
      HIP_TRY(hipStreamWaitEvent(e->main_s, e->ev_rank[e->rank_seq & 1u], 0));
      e->rank_seq = 0;
    }
    launch_pipeline(aa, e->main_s, ev_start);
    HIP_TRY(hipGetLastError());
  }
  if (ra.wg1 + ra.wg2) {
    HIP_TRY(hipEventRecord(e->ev_rank[a.launch_seq & 1u], e->rank_s));
    e->rank_seq = a.launch_seq;
  }
  return RMQ_OK;
}

int issue(rmq_engine* e, const PipeArgs& a, hipEvent_t ev_start) {
  if (e->knob.split && !a.outidx) return issue_split(e, a, ev_start);
  launch_pipeline(a, e->main_s, ev_start);
  HIP_TRY(hipGetLastError());
  return RMQ_OK;
}

// After a launch with a stage 3: the state sets swap, host batches' out offsets start back, and the
// launch is marked as the one that completes the group's tickets.
int after_apply(rmq_engine* e, const Stages& g) {
  e->applied++;
  const StateSet& now = e->sets[e->applied & 1u];
  e->st.leo = now.leo;
  e->st.used = now.used;
  for (uint32_t j = 0; j < g.s3->nb; ++j) {
    const InFlight& f = g.s3->b[j];
    if (f.host_out && f.b.n)
      HIP_TRY(hipMemcpyAsync(f.host_out, f.b.out_offsets, f.b.n * 8ull, hipMemcpyDeviceToHost, e->main_s));
  }
  // this launch also completes the empty tickets up to the next group's first one
  const GroupFlight* next = g.s2 ? g.s2 : g.s1;
  const uint64_t hi = next ? next->b[0].ticket - 1 : e->last_ticket;
  e->marks.emplace_back(hi, e->launch_seq);
  return RMQ_OK;
}

// One pipeline launch.
int launch_stages(rmq_engine* e, const Stages& g) {
  PipeArgs a{};
  pipe_args_common(e, a);
  int rc = stage_groups(e, a, g);
  if (rc) return rc;
  repl_pipe_args(e, a, g.s2, g.s3);
  rc = repl_before_launch(e, a);  // followers' acks of the group applied three launches ago
  if (rc) return rc;
  const RolePlan plan = plan_roles(e->knob, launch_shape(e, a, g));  // (neither hook reads a role's count)
  set_roles(a, plan);
  const hipEvent_t ev_start = number_launch(e, a, plan, g.s3);
  if (e->knob.trace)  // RMQ_TRACE: the roles of every launch (diagnostics only)
    std::fprintf(stderr, "rmq launch %llu: s1 %u batches %u wgs | s2 %u batches %u wgs | parts %u wgs | s3 %u batches %u wgs + %u big | s4 %u batches\n",
                 (unsigned long long)a.launch_seq, a.g1.nb, a.wg1, a.g2.nb, a.wg2, a.wgp, a.g3.nb, a.wg3, a.wgb, a.g4.nb);
  rc = issue(e, a, ev_start);
  if (!rc && g.s3) rc = after_apply(e, g);
  return rc ? rc : repl_after_launch(e, g.s2, g.s3);
}

// One launch: ranks the group being formed (if any) and advances the groups ahead of it.
int close_group(rmq_engine* e) {
  const GroupFlight* s1 = e->forming.nb ? &e->forming : nullptr;
  // bounded run-ahead (RMQ_AHEAD launches queued at most, no transport): a fetch or an offset
  // commit is ordered after the launches issued before it, so an unbounded queue would make its
  // latency grow with how far the host runs ahead (device batches are never waited for otherwise).
  // Launch L's first lane reports L - 1 complete (done word).
  if (e->knob.max_ahead && !e->repl) {
    const uint64_t ahead = e->knob.max_ahead, need = e->launch_seq + 1 > ahead ? e->launch_seq + 1 - ahead : 0;
    // poll the done word (host memory); the stream itself only now and then (a faulted launch
    // never moves the word: its sticky error ends the wait)
    for (uint32_t spin = 1; need > __atomic_load_n(e->done_host, __ATOMIC_ACQUIRE); ++spin) {
      if ((spin & 1023u) == 0) {
        const hipError_t q = hipStreamQuery(e->main_s);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) return hip_fail(q);
      }
      __builtin_ia32_pause();
    }
  }
  int rc = launch_stages(e, Stages{s1, e->has1 ? &e->g1 : nullptr, e->has2 ? &e->g2 : nullptr,
                                   e->has3 ? &e->g3 : nullptr});
  if (rc) return rc;
  e->has3 = e->has2;
  e->g3 = e->g2;
  if (e->has3) e->g3_seq = e->launch_seq;  // the launch that applied it
  e->has2 = e->has1;
  e->g2 = e->g1;
  e->has1 = s1 != nullptr;
  if (s1) e->g1 = e->forming;
  e->forming = GroupFlight{};
  return RMQ_OK;
}

// Has the launch with sequence number L completed?
bool launch_done(rmq_engine* e, uint64_t L) {
  if (L <= __atomic_load_n(e->done_host, __ATOMIC_ACQUIRE)) return true;
  return hipStreamQuery(e->main_s) == hipSuccess;
}

// Completed launches: the tickets they complete, and those host batches' out offsets from their
// pinned slots into the callers' buffers.
void collect_done(rmq_engine* e) {
  while (!e->marks.empty() && launch_done(e, e->marks.front().second)) {
    e->done_ticket = std::max(e->done_ticket, e->marks.front().first);
    e->marks.pop_front();
  }
  for (Staging& sg : e->staging)
    if (sg.user_out && sg.ticket <= e->done_ticket) {
      std::memcpy(sg.user_out, sg.h_out, (size_t)sg.out_n * 8);
      sg.user_out = nullptr;
    }
}

// Ticket completion: 1 complete, 0 applied by a launch still running, -1 not applied yet.
int ticket_state(rmq_engine* e, uint64_t t) {
  collect_done(e);
  if (t <= e->done_ticket) return 1;
  if (!e->marks.empty() && t <= e->marks.back().first) return 0;
  return -1;
}

// Block until ticket t (issued) is applied and complete.
int wait_ticket(rmq_engine* e, uint64_t t) {
  int s = ticket_state(e, t);
  if (s < 0) {
    if (e->repl) return RMQ_PENDING;  // a flush is collective with a transport: rmq_sync on every rank
    int rc = flush(e);
    if (rc) return rc;
    s = ticket_state(e, t);
  }
  if (s == 0) {  // wait for the launch that completes t, not for everything queued behind it
    uint64_t L = e->launch_seq;
    for (const auto& m : e->marks)
      if (m.first >= t) {
        L = m.second;
        break;
      }
    // the done word only moves while launches succeed: a faulted stream (sticky error) ends the wait
    while (L > __atomic_load_n(e->done_host, __ATOMIC_ACQUIRE)) {
      const hipError_t q = hipStreamQuery(e->main_s);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) return hip_fail(q);
      std::this_thread::yield();
    }
    ticket_state(e, t);
  }
  return RMQ_OK;
}

// rmq_append's checks of the caller's batch, in this order (host batches: payload ranges like the
// oracle, RMQ_EINVAL).
int check_batch(const rmq_engine* e, const rmq_batch* b, const uint64_t* out_offsets) {
  const uint32_t n = b->n;
  if (n > e->cfg.max_batch_records) return RMQ_ENOSPC;
  if (b->payload_bytes > e->cfg.max_batch_bytes) return RMQ_ENOSPC;
  if (b->mem != RMQ_MEM_HOST && b->mem != RMQ_MEM_DEVICE && b->mem != RMQ_MEM_PINNED) return RMQ_EINVAL;
  if (n && (!b->pidx || !b->len || !out_offsets)) return RMQ_EINVAL;
  if (b->payload_bytes && !b->payload) return RMQ_EINVAL;
  if (b->mem == RMQ_MEM_DEVICE && (reinterpret_cast<uintptr_t>(b->payload) & 3u)) return RMQ_EINVAL;
  if (b->mem != RMQ_MEM_HOST) return RMQ_OK;
  uint64_t run = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t off = b->payload_off ? b->payload_off[i] : run;
    run += b->len[i];
    if (b->len[i] && (off > b->payload_bytes || b->len[i] > b->payload_bytes - off)) return RMQ_EINVAL;
  }
  return RMQ_OK;
}

// A host batch's staging slot, free for ticket t, and where its sections lie in the slot's block
// (pidx | len | payload_off | payload, 16-byte aligned).
struct StageSlot {
  Staging* sg;
  uint64_t o_len, o_poff, o_pay;
};

int staging_slot(rmq_engine* e, const rmq_batch* b, uint64_t t, StageSlot* s) {
  Staging& sg = e->staging[t % e->staging.size()];
  if (sg.ticket) {  // the batch that used this staging slot must be complete
    int rc = wait_ticket(e, sg.ticket);
    if (rc) return rc;
    collect_done(e);
  }
  const uint64_t NB = e->cfg.max_batch_records, cap = 32ull * NB + e->cfg.max_batch_bytes + 64;
  if (!sg.d_blk)  // the first host batch sets up every slot (allocation synchronizes the device)
    for (Staging& z : e->staging) {
      int rc = dalloc(&z.d_blk, cap);
      if (!rc) rc = dalloc(&z.d_out, NB);
      if (rc) return rc;
      HIP_TRY(hipHostMalloc((void**)&z.h_blk, cap, 0));
      HIP_TRY(hipHostMalloc((void**)&z.h_out, NB * 8, 0));
      HIP_TRY(hipEventCreateWithFlags(&z.ev_in, hipEventDisableTiming));
    }
  const uint64_t sec32 = (4ull * b->n + 15) & ~15ull;
  s->sg = &sg;
  s->o_len = sec32;
  s->o_poff = 2 * sec32;
  s->o_pay = s->o_poff + (b->payload_off ? (8ull * b->n + 15) & ~15ull : 0ull);
  return RMQ_OK;
}

// Caller-pinned sections: one DMA each straight into the device slot, no host copy.
int fill_pinned(rmq_engine* e, const rmq_batch* b, uint64_t t, const StageSlot& s) {
  uint8_t* const d = s.sg->d_blk;
  const uint64_t n = b->n;
  s.sg->ticket = t;
  HIP_TRY(hipMemcpyAsync(d, b->pidx, 4 * n, hipMemcpyHostToDevice, e->copy_s));
  HIP_TRY(hipMemcpyAsync(d + s.o_len, b->len, 4 * n, hipMemcpyHostToDevice, e->copy_s));
  if (b->payload_off) HIP_TRY(hipMemcpyAsync(d + s.o_poff, b->payload_off, 8 * n, hipMemcpyHostToDevice, e->copy_s));
  if (b->payload_bytes)
    HIP_TRY(hipMemcpyAsync(d + s.o_pay, b->payload, b->payload_bytes, hipMemcpyHostToDevice, e->copy_s));
  return RMQ_OK;
}

// Pageable arrays: packed into the slot's pinned block by the copy pool, then one DMA.
int fill_packed(rmq_engine* e, const rmq_batch* b, uint64_t t, const StageSlot& s) {
  if (!e->copy_pool) {
    // RMQ_COPY_THREADS: packing threads besides the caller's (default min(7, cores / 2))
    const char* env = std::getenv("RMQ_COPY_THREADS");
    const unsigned hc = std::max(1u, std::thread::hardware_concurrency());
    unsigned k = env ? (unsigned)std::atoi(env) : std::min(7u, hc / 2u);
    e->copy_pool = new (std::nothrow) CopyPool(std::min(k, 64u));
    if (!e->copy_pool) return RMQ_ENOMEM;
  }
  uint8_t* const h = s.sg->h_blk;
  const uint64_t n = b->n;
  std::vector<CopyPool::Seg> segs = {{h, reinterpret_cast<const uint8_t*>(b->pidx), 4 * n},
                                     {h + s.o_len, reinterpret_cast<const uint8_t*>(b->len), 4 * n}};
  if (b->payload_off) segs.push_back({h + s.o_poff, reinterpret_cast<const uint8_t*>(b->payload_off), 8 * n});
  if (b->payload_bytes) segs.push_back({h + s.o_pay, b->payload, b->payload_bytes});
  s.sg->ticket = t;
  e->copy_pool->run(segs, 512u << 10);
  HIP_TRY(hipMemcpyAsync(s.sg->d_blk, h, s.o_pay + b->payload_bytes, hipMemcpyHostToDevice, e->copy_s));
  return RMQ_OK;
}

// A host batch (pageable or pinned) goes to its staging slot on the copy stream, which the pipeline
// stream waits for; f then names the slot's device arrays.
int stage_host_batch(rmq_engine* e, const rmq_batch* b, uint64_t* out_offsets, uint64_t t, InFlight& f) {
  const bool pinned = b->mem == RMQ_MEM_PINNED;
  StageSlot s{};
  int rc = staging_slot(e, b, t, &s);
  if (!rc) rc = pinned ? fill_pinned(e, b, t, s) : fill_packed(e, b, t, s);
  if (rc) return rc;
  Staging& sg = *s.sg;
  HIP_TRY(hipEventRecord(sg.ev_in, e->copy_s));
  HIP_TRY(hipStreamWaitEvent(e->main_s, sg.ev_in, 0));  // before the group's first launch
  if (e->rank_s) HIP_TRY(hipStreamWaitEvent(e->rank_s, sg.ev_in, 0));  // (its ranking, split launches)
  f.b.pidx = reinterpret_cast<const uint32_t*>(sg.d_blk);
  f.b.len = reinterpret_cast<const uint32_t*>(sg.d_blk + s.o_len);
  f.b.poff = b->payload_off ? reinterpret_cast<const uint64_t*>(sg.d_blk + s.o_poff) : nullptr;
  f.b.payload = sg.d_blk + s.o_pay;
  f.b.out_offsets = sg.d_out;
  f.host_out = pinned ? out_offsets : sg.h_out;  // pinned: the DMA writes the caller's array
  sg.user_out = pinned ? nullptr : out_offsets;
  sg.out_n = b->n;
  return RMQ_OK;
}

// The batch joins the forming group, which a full group (or one out of tiles) closes.
int join_group(rmq_engine* e, const InFlight& f) {
  if (e->forming.nb && e->forming.tiles + f.b.tiles > e->max_group_tiles) {  // (never with a transport)
    int rc = close_group(e);
    if (rc) return rc;
  }
  GroupFlight& fg = e->forming;
  if (!fg.nb) fg.set = (uint32_t)(e->groups++ % kSets);
  fg.b[fg.nb++] = f;
  fg.tiles += f.b.tiles;
  fg.tasks += (f.b.n + kTaskRecs - 1) / kTaskRecs;
  return fg.nb >= e->group_max ? close_group(e) : RMQ_OK;
}

}  // namespace

// Push everything through stage 3 (at most three launches). The stage-3 launch of a group applies
// its retention too unless a partition's group outgrew the entries written before it
// (pipeline.hip partition_threads): drain() then adds the stage-4 launch. With a transport a flush
// is collective and every rank makes the same launches: stage 4 always.
int flush(rmq_engine* e) {
  while (e->forming.nb || e->has1 || e->has2 || (e->has3 && e->repl)) {
    int rc = close_group(e);
    if (rc) return rc;
  }
  return RMQ_OK;
}

int drain(rmq_engine* e) {
  int rc = flush(e);
  if (!rc) rc = repl_drain(e);  // the remaining replication rounds and their acks
  if (rc) return rc;
  rmq_engine::ProfRegion& r = e->region;
  if (e->profile && r.started && !r.ended) {
    HIP_TRY(hipEventRecord(r.t1, e->main_s));
    r.ended = true;
  }
  rc = stream_wait(e->main_s);
  if (rc) return rc;
  if (e->has3) {  // the last group's retention: finished by its own launch unless ret_late names it
    if (__atomic_load_n(e->done_host + 1, __ATOMIC_ACQUIRE) >= e->g3_seq) {
      rc = close_group(e);  // stage 4 alone
      if (rc) return rc;
      if (e->profile && r.ended) HIP_TRY(hipEventRecord(r.t1, e->main_s));
      rc = stream_wait(e->main_s);
      if (rc) return rc;
    } else {
      e->set_reset |= 1u << e->g3.set;  // its stage 4 would reset the set's list and sums
    }
    e->has3 = false;
  }
  collect_done(e);
  return RMQ_OK;
}

// The last applied group's retention, where its own launch stopped early (late_retention_kernel),
// before a fetch or a state read ordered after that launch; once per applied group.
int late_retention(rmq_engine* e) {
  if (!e->has3 || e->late_done == e->g3_seq) return RMQ_OK;
  LateArgs a{};
  a.st = e->st;
  a.bcum = e->scratch[e->g3.set].bcum;
  a.totals = e->scratch[e->g3.set].totals;
  a.rlate = e->d_rlate;
  a.nb = e->g3.nb;
  launch_late_retention(a, e->main_s);
  HIP_TRY(hipGetLastError());
  e->late_done = e->g3_seq;
  return RMQ_OK;
}

// Wait for everything issued on the pipeline stream, without flushing batches that are still
// forming or in the pipeline's earlier stages (reads of committed state, consumer commits).
int quiesce(rmq_engine* e) {
  int rc0 = late_retention(e);
  if (rc0) return rc0;
  int rc = stream_wait(e->main_s);
  if (rc) return rc;
  collect_done(e);
  return RMQ_OK;
}

// Drain, or with a replication transport (where a flush is collective: rmq_sync) just wait for
// what is issued: device memory management and profiling calls.
int settle(rmq_engine* e) { return e->repl ? quiesce(e) : drain(e); }

void dump_stamps(rmq_engine* e) {
  const RolePlan& plan = e->stamps_plan;
  const uint32_t nwg = plan.wg1 + plan.wg2 + plan.wgp + plan.wg3;
  if (!e->stamps_path || !e->d_stamps || !nwg) return;
  // the launch's layout: waves per workgroup of its variant, roles in dispatch order
  const uint32_t wpg = (e->repl ? kPipeThreadsXR : kPipeThreads) / 64u;
  std::vector<uint64_t> h((size_t)nwg * wpg * 8);
  if (hipMemcpy(h.data(), e->d_stamps, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
  FILE* f = std::fopen(e->stamps_path, "w");
  if (!f) return;
  std::fprintf(f, "wg,wave,stage,t0,t1,t2,t3,t4,t5,t6,t7\n");
  for (uint32_t g = 0; g < nwg; ++g) {
    const int stage = role_of_block(plan, g);  // (4: partitions)
    for (uint32_t w = 0; w < wpg; ++w) {
      std::fprintf(f, "%u,%u,%d", g, w, stage);
      for (int k = 0; k < 8; ++k) std::fprintf(f, ",%llu", (unsigned long long)h[((size_t)g * wpg + w) * 8 + k]);
      std::fprintf(f, "\n");
    }
  }
  std::fclose(f);
}

void staging_free(rmq_engine* e) {
  delete e->copy_pool;
  e->copy_pool = nullptr;
  for (Staging& sg : e->staging) {  // (hipFree and hipHostFree take null)
    hipFree(sg.d_blk), hipFree(sg.d_out), hipHostFree(sg.h_blk), hipHostFree(sg.h_out);
    if (sg.ev_in) hipEventDestroy(sg.ev_in);
  }
  e->staging.clear();
}

}  // namespace rmq

extern "C" {

int rmq_append(rmq_engine* e, const rmq_batch* b, uint64_t* out_offsets, uint64_t* ticket) {
  if (!e || !b || !ticket) return RMQ_EINVAL;
  EngineLock g(e);
  int rc = check_batch(e, b, out_offsets);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(e->device));

  // the ticket is taken only once nothing below can fail short of a device error: the staging
  // slot's wait and the first host batch's allocations come first (with a transport a used-up
  // ticket without a queued batch would leave this rank's groups out of step with its peers')
  const uint64_t t = e->last_ticket + 1;
  // an empty batch still takes its place in a launch group (0 tiles, 0 tasks): every rank of a
  // replication transport forms the same groups from the same number of calls
  InFlight f;
  f.ticket = t;
  f.b.pidx = b->pidx;
  f.b.len = b->len;
  f.b.poff = b->payload_off;
  f.b.payload = b->payload;
  f.b.payload_bytes = b->payload_bytes;
  f.b.out_offsets = out_offsets;
  f.b.n = b->n;
  f.b.tiles = (b->n + kTileRecs - 1) / kTileRecs;
  if (b->mem != RMQ_MEM_DEVICE && b->n) {
    rc = stage_host_batch(e, b, out_offsets, t, f);
    if (rc) return rc;
  }
  e->last_ticket = t;
  *ticket = t;
  e->ticket_n[t % kStatsRing] = b->n;
  return join_group(e, f);
}

int rmq_poll_commit(rmq_engine* e, uint64_t ticket, uint64_t* commit_out, uint64_t* hw_out) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  if (ticket & RMQ_TICKET_OFFSETS) {
    HIP_TRY(hipSetDevice(e->device));
    return poll_offsets(e, ticket);
  }
  if (ticket > e->last_ticket) return RMQ_EINVAL;  // never issued
  HIP_TRY(hipSetDevice(e->device));
  if (ticket) {
    int s = ticket_state(e, ticket);
    if (s < 0 && !e->repl) {
      int rc = flush(e);  // a poll pushes the batch through the remaining stages
      if (rc) return rc;
      s = ticket_state(e, ticket);
    }
    if (s <= 0) return RMQ_PENDING;
  }
  int rc = check_err(e);
  if (rc) return rc;
  const size_t P = e->cfg.num_partitions;
  if (commit_out || hw_out) {
    rc = settle(e);  // snapshot after everything submitted (applied, with a transport)
    if (rc) return rc;
    if (commit_out) HIP_TRY(hipMemcpy(commit_out, e->st.commit, P * 8, hipMemcpyDeviceToHost));
    if (hw_out) HIP_TRY(hipMemcpy(hw_out, e->st.hw, P * 8, hipMemcpyDeviceToHost));
  }
  return RMQ_OK;
}

int rmq_ticket_stats(rmq_engine* e, uint64_t ticket, rmq_append_stats* out) {
  if (!e || !out) return RMQ_EINVAL;
  EngineLock g(e);
  if (!ticket || ticket > e->last_ticket || e->last_ticket - ticket >= kStatsRing) return RMQ_EINVAL;
  HIP_TRY(hipSetDevice(e->device));
  int rc = wait_ticket(e, ticket);
  if (rc) return rc;  // RMQ_PENDING with a transport until an rmq_sync applied the ticket
  const uint32_t n = e->ticket_n[ticket % kStatsRing];
  const uint32_t tasks = (n + kTaskRecs - 1) / kTaskRecs;
  std::vector<uint4> ts(tasks ? tasks : 1);
  if (tasks)
    HIP_TRY(hipMemcpy(ts.data(), e->d_stats + (size_t)(ticket % kStatsRing) * e->max_tasks,
                      tasks * sizeof(uint4), hipMemcpyDeviceToHost));
  std::memset(out, 0, sizeof *out);
  out->records = n;
  for (uint32_t k = 0; k < tasks; ++k) {
    out->appended += ts[k].x;
    out->rejected_not_leader += ts[k].y;
    out->rejected_no_partition += ts[k].z;
    out->rejected_no_space += ts[k].w & 0xFFFFu;
    out->rejected_invalid += ts[k].w >> 16;
  }
  return check_err(e);
}

int rmq_sync(rmq_engine* e) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  return begin_call(e, drain);
}

}  // extern "C"
