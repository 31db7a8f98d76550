// engine_internal.hpp — the engine object shared by the host-side translation units
// (engine.cpp: creation, destruction, memory, profiling and transport attach; append.cpp: the append
// pipeline and its tickets; offsets.cpp: consumer-offset commits and acks; control.cpp: roles,
// placement, votes, ring moves; inspect.cpp: read-backs and fault injection; fetch.cpp: the fetch calls; lag.cpp: rmq_lag; unpack.cpp: rmq_unpack;
// audit.cpp: scrub, repair, reindex, remote repair, restore; replication.cpp: replica-log rounds;
// repair_remote.cpp: the rounds of rmq_repair_remote). launch_plan.hpp holds the knobs and the role
// grid of a launch, repl_plan.hpp the replication lists, buffer bounds and round layout; both are
// free of the device runtime and checked by stand-alone programs under tools/.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <chrono>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ripplemq_engine.h"
#include "device_common.hpp"
#include "kernels.hpp"
#include "launch_plan.hpp"
#include "repl_plan.hpp"
#include "transport.hpp"

using namespace rmq;

namespace rmq {

constexpr uint32_t kStatsRing = 64;                                // tickets whose stats stay readable
constexpr uint32_t kMaxBatchRecords = kMaxTiles * kTileRecs;       // 524288
// pipeline scratch sets: a group's set lives from its stage 1 (launch k) to the application of its
// followers' acks (launch k + 5 with a replication transport), so six sets rotate
constexpr uint32_t kSets = 6;
static_assert(kPlanMaxWorld == kMaxWorld, "repl_plan.hpp sizes its per-peer arrays for kMaxWorld ranks");
// rmq_repair_remote's control words (rmq_engine::RemoteRepair::words): the words sent [2 * kMaxWorld]
// and received [2 * kMaxWorld], RemoteReqArgs::ctr [2 * kMaxWorld + 1], RemoteServeArgs::tot [3 * kMaxWorld]
constexpr uint32_t kRemoteWSend = 0, kRemoteWRecv = 2 * kMaxWorld, kRemoteWCtr = 4 * kMaxWorld,
                   kRemoteWTot = 6 * kMaxWorld + 1, kRemoteWords = 9 * kMaxWorld + 1;

struct EvPair {
  hipEvent_t a = nullptr, b = nullptr;
};

// Device buffers a subsystem reallocates as a set: each is noted where it is allocated (the address
// of its pointer) and freed, its pointer nulled, from this record alone (hipFree takes a null).
struct DevRecord {
  std::vector<void**> ptrs;
  template <typename T>
  void note(T** p) { ptrs.push_back(reinterpret_cast<void**>(p)); }
  void free_all() {
    for (void** p : ptrs) {
      hipFree(*p);
      *p = nullptr;
    }
    ptrs.clear();
  }
};

// Device staging of host-memory batches.
// Host threads that pack a host batch into its pinned staging slot: one memcpy split into chunks
// that the workers and the submitting thread take in turn (a single thread fills pinned memory at
// ~7 GB/s, a quarter of what the DMA behind it moves).
class CopyPool {
 public:
  struct Seg {
    uint8_t* d;
    const uint8_t* s;
    size_t n;
  };
  explicit CopyPool(unsigned workers) {
    for (unsigned i = 0; i < workers; ++i) th_.emplace_back([this] { work(); });
  }
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> g(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (std::thread& t : th_) t.join();
  }
  // Copy every segment (chunked), using the workers and the calling thread; returns when done.
  void run(const std::vector<Seg>& segs, size_t chunk) {
    chunks_.clear();
    for (const Seg& g : segs)
      for (size_t o = 0; o < g.n; o += chunk) chunks_.push_back({g.d + o, g.s + o, std::min(chunk, g.n - o)});
    if (th_.empty() || chunks_.size() < 2) {
      for (const Seg& c : chunks_) std::memcpy(c.d, c.s, c.n);
      return;
    }
    next_.store(0);
    left_.store(chunks_.size());
    {
      std::lock_guard<std::mutex> g(m_);
      ++gen_;
    }
    cv_.notify_all();
    take();
    std::unique_lock<std::mutex> g(m_);
    done_.wait(g, [this] { return left_.load() == 0; });
  }
  unsigned workers() const { return (unsigned)th_.size(); }

 private:
  void take() {
    for (size_t i; (i = next_.fetch_add(1)) < chunks_.size();) {
      std::memcpy(chunks_[i].d, chunks_[i].s, chunks_[i].n);
      if (left_.fetch_sub(1) == 1) {
        std::lock_guard<std::mutex> g(m_);
        done_.notify_all();
      }
    }
  }
  void work() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [&] { return stop_ || gen_ != seen; });
        if (stop_) return;
        seen = gen_;
      }
      take();
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  std::vector<Seg> chunks_;
  std::atomic<size_t> next_{0}, left_{0};
  uint64_t gen_ = 0;
  bool stop_ = false;
};

// A host batch's slot: the caller's arrays are packed into pinned memory (pidx | len | payload_off |
// payload, 16-byte aligned sections) and cross PCIe as one DMA on the copy stream, which the
// pipeline stream waits for; the out offsets come back into pinned memory and reach the caller's
// buffer when the ticket is seen complete.
struct Staging {
  uint8_t* h_blk = nullptr;    // pinned, packed batch
  uint8_t* d_blk = nullptr;    // device copy
  uint64_t* h_out = nullptr;   // pinned out offsets
  uint64_t* d_out = nullptr;
  hipEvent_t ev_in = nullptr;  // the DMA of the batch is done
  uint64_t ticket = 0;         // last ticket that used it
  uint64_t* user_out = nullptr;  // caller's out_offsets, pending copy-out
  uint32_t out_n = 0;
};

// A batch inside the launch pipeline.
struct InFlight {
  uint64_t ticket = 0;
  PipeBatch b{};
  uint64_t* host_out = nullptr;  // host batches: caller's out_offsets
};

// A group of consecutive batches moving through the pipeline together (one launch per stage).
struct GroupFlight {
  uint32_t nb = 0, tiles = 0, tasks = 0;
  uint32_t set = 0;              // scratch set = group number % kSets
  InFlight b[kMaxGroup];
};

// Replica-log rounds over a transport (replication.cpp, FORMAT.md §9): per scratch set, the
// group's outbox and inbox and the exchange's events.
struct XchgSet {
  uint8_t* outbox = nullptr;   // region for destination d at d * dcap
  uint8_t* inbox = nullptr;    // received regions packed in source order
  XEntry* xe = nullptr;        // [n_out]
  XCatch* xc = nullptr;        // [n_out] catch-up list (plan -> stage-3 catch-up waves)
  uint32_t* xc_n = nullptr;    // [2]
  uint64_t* sizes = nullptr;   // device [4 * world]: send sizes (plan), receive sizes (exchange)
  uint64_t* h_sizes = nullptr; // pinned copy
  uint64_t* ackout = nullptr;  // [n_in][2]
  uint64_t* ackin = nullptr;   // [n_out][2]
  uint64_t* rowv = nullptr;    // [n_out] consumer-offset row version each entry of the round carries
  uint32_t* count = nullptr;   // stage-2 arrival counter
  hipEvent_t ev_s2 = nullptr, ev_s3 = nullptr, ev_sz = nullptr, ev_x = nullptr;
  uint64_t applied_launch = 0; // launch that ran the group's stage 3
  uint64_t round = 0;          // the group's round number (FORMAT.md §9)
};

struct Replication {
  Transport* xport = nullptr;
  uint32_t world = 1, rank = 0;
  hipStream_t xchg_s = nullptr;
  ReplLists lists;  // the placement's out / in lists (plan_lists), replaced by every placement call
  DevRecord placed;  // the device buffers sized by the placement (placed_alloc in replication.cpp)
  uint32_t* d_xo_p = nullptr;
  uint32_t* d_xo_start = nullptr;
  uint64_t* d_keysum = nullptr;
  uint64_t* d_keysum_in = nullptr;  // [world] key sums of the in lists (the follower's side)
  uint32_t* d_outidx = nullptr;  // [P][RF]
  uint32_t* d_xi_p = nullptr;
  uint32_t* d_xi_slot = nullptr;
  uint32_t* d_xi_start = nullptr;
  uint32_t* d_xo_slot = nullptr;  // [n_out]
  uint32_t* d_bad = nullptr;     // [n_in]
  uint32_t* d_acc = nullptr;     // [n_in]
  uint64_t* d_base = nullptr;    // [n_in][2] IngestArgs::base
  uint64_t* d_cdesc = nullptr;   // [n_in][4] IngestArgs::cdesc
  uint32_t* d_items = nullptr;   // [items_cap][2] follower copy work items
  uint32_t* d_nitems = nullptr;  // [2][1 + kMaxWorld]: copy items allocated, structural flag per source;
                                 // rounds alternate halves, each round's prepare clears the other
  uint32_t nitems_par = 0;
  uint64_t* d_counters = nullptr;  // [7]: follower [0..4) (IngestArgs), leader [4..7) (XPlanArgs)
  uint64_t* d_lastg = nullptr;     // [P] record bytes / 16 of the last group applied (PipeArgs::lastg)
  uint64_t* d_shake = nullptr;     // [8 * kMaxWorld] the placement handshake's words, made at attach
  // leader catch-up state per out entry (FORMAT.md §9 v3)
  uint64_t* d_xnext = nullptr;   // [n_out][2]
  uint64_t* d_xreq = nullptr;    // [n_out][4]
  uint64_t* d_xcu = nullptr;     // [n_out]
  XDecision* d_xdec = nullptr;   // [n_out]
  uint64_t* d_xtot = nullptr;    // [n_out]
  uint32_t* d_dflag = nullptr;   // [world]
  uint64_t* d_nout = nullptr;    // [n_out][2] commit notices sent {commit, term} (FORMAT.md §9 v4)
  uint64_t* d_nin = nullptr;     // [n_in][2] commit notices received
  uint64_t* d_eackv = nullptr;   // [n_out] row version each follower acknowledged (offset tickets)
  hipEvent_t ev_notice = nullptr;
  uint64_t dcap = 0;             // outbox bytes per destination
  uint64_t reserve = 0;          // catch-up bytes per destination
  uint64_t items_cap = 0;
  uint64_t planned = 0;          // rounds planned (the next plan's round number)
  uint64_t out_cap = 0, in_cap = 0;
  XchgSet sets[kSets];
  std::deque<uint32_t> sized;    // sets whose size exchange is posted, data exchange not yet
  std::deque<uint32_t> acking;   // sets whose data exchange is posted, acks not yet applied
  uint64_t rounds = 0, bytes_sent = 0, bytes_recv = 0;
  uint64_t host_waits = 0, host_wait_ns = 0;  // post_round found the sizes not landed yet
  uint32_t last_set = ~0u;       // set of the last posted round (rmq_read_outbox)
  // fault injection (rmq_fault_drop_rounds): the rounds of the next `drop_n` groups whose first
  // ticket is at least `drop_from` send empty regions
  uint64_t drop_from = 0;
  uint32_t drop_n = 0;
  // rmq_fault_isolate: the next iso_n[q] rounds (groups from ticket iso_from[q] on) to q are lost
  uint64_t iso_from[kMaxWorld] = {};
  uint32_t iso_n[kMaxWorld] = {};
  uint32_t cut_notice = 0;      // rmq_fault_cut: bit q, the next drain's commit notices to q are lost
  uint64_t stamp = 0;           // round stamp: the last round posted for ingest, + 1 (heard words)
  std::chrono::steady_clock::time_point stamp_time[64];  // when stamp s was posted, at [s % 64]
  // rmq_fault_corrupt: the next round to destination q flips the byte at flip_at[q]
  bool flip[kMaxWorld] = {};
  int64_t flip_at[kMaxWorld] = {};
};

// The arguments of one Transport::exchange: for every peer q the bytes sent from sb[q] and received
// into rb[q] (this rank's own entries: 0 bytes).
struct Exchange {
  void* sb[kMaxWorld];
  void* rb[kMaxWorld];
  uint64_t sn[kMaxWorld], rn[kMaxWorld];
  void peer(uint32_t q, void* s, uint64_t s_bytes, void* r, uint64_t r_bytes) {
    sb[q] = s, sn[q] = s_bytes, rb[q] = r, rn[q] = r_bytes;
  }
  int post(Replication* r) const { return r->xport->exchange(sb, sn, rb, rn, r->xchg_s); }
};
// n bytes to and from every peer: peer q's at element q * stride of send and of recv.
template <typename T>
Exchange fixed_swap(const Replication* r, T* send, T* recv, uint32_t stride, uint64_t n) {
  Exchange x;
  for (uint32_t q = 0; q < r->world; ++q)
    x.peer(q, send + (size_t)q * stride, q == r->rank ? 0 : n, recv + (size_t)q * stride, q == r->rank ? 0 : n);
  return x;
}

}  // namespace rmq

namespace rmq {
// Ring space of the pool (FORMAT.md §2): power-of-two blocks aligned to their size, free lists per
// size class, blocks split from larger free ones or cut from the unused tail; no coalescing.
struct SegPool {
  uint64_t size = 0, bump = 0;
  std::vector<uint64_t> free[64];
  void give(uint64_t off, uint64_t end) {  // [off, end) into the free lists as aligned blocks
    while (off < end) {
      uint32_t lg = off ? (uint32_t)__builtin_ctzll(off) : 63u;
      while ((1ull << lg) > end - off) --lg;
      free[lg].push_back(off);
      off += 1ull << lg;
    }
  }
  bool alloc(uint32_t lg, uint64_t* off) {
    for (uint32_t k = lg; k < 64; ++k) {
      if (free[k].empty()) continue;
      const uint64_t o = free[k].back();
      free[k].pop_back();
      for (uint32_t q = k; q > lg; --q) free[q - 1].push_back(o + (1ull << (q - 1)));  // split
      *off = o;
      return true;
    }
    const uint64_t a = (bump + (1ull << lg) - 1) & ~((1ull << lg) - 1);
    if (a + (1ull << lg) > size) return false;
    give(bump, a);
    bump = a + (1ull << lg);
    *off = a;
    return true;
  }
  void release(uint32_t lg, uint64_t off) { free[lg].push_back(off); }
};
}  // namespace rmq

struct rmq_engine {
  rmq_config cfg{};
  std::mutex mu;
  int device = 0;
  uint32_t cu_count = 0;
  char dev_name[256] = {0};

  // ---- knobs: read from the environment by rmq_create, never afterwards (launch_plan.hpp)
  rmq::Knobs knob;

  // ---- streams and events
  hipStream_t main_s = nullptr;  // the pipeline stream
  hipStream_t rank_s = nullptr;  // the ranking launches of split launches (Knobs::split)
  hipStream_t copy_s = nullptr;  // host batches and fetch requests: pinned -> device DMA
  hipStream_t fetch_out_s = nullptr;  // fetch results (and host outputs) -> host, after the kernels:
                                      // a fetch's result copy overlaps the next fetch's kernels
  hipEvent_t ev_main = nullptr;
  hipEvent_t ev_rank[2] = {nullptr, nullptr};  // rank launch L recorded in slot L & 1
  hipEvent_t ev_pre_rank = nullptr;            // main_s before a rank launch
  uint64_t rank_seq = 0;        // the last launch that had a rank launch (0: none)
  std::vector<hipEvent_t> ev_pool;

  // ---- device state
  DevState st{};            // leo/used point at sets[applied & 1]
  StateSet sets[2]{};
  uint64_t applied = 0;     // stage-3 launches issued
  CrcConsts* d_crc = nullptr;
  uint32_t* d_rlate = nullptr;  // [P] partitions whose retention of the applied group stopped early
  uint4* d_stats = nullptr;  // [kStatsRing][max tasks]
  PipeScratch scratch[kSets]{};
  rmq::SegPool pool;         // ring space of each replica region
  // device and page-locked memory that lives as long as the engine, recorded where it is allocated
  // (owned_dalloc, owned_host_alloc) and freed from these lists alone
  std::vector<void*> owned_dev, owned_host;

  // ---- pipeline groups and launch counters: the group being formed, then groups ranked (need
  // stage 2), scanned (need stage 3) and applied (need stage 4)
  GroupFlight forming, g1, g2, g3;
  bool has1 = false, has2 = false, has3 = false;
  uint64_t g3_seq = 0;     // the launch that applied g3 (its retention is late if done_host[1] >= it)
  uint64_t late_done = 0;  // the applied group (by launch) whose late retention ran (late_retention)
  uint32_t set_reset = 0;  // scratch sets whose large-record list and batch sums the next stage 1 zeroes
  uint32_t group_max = 2;       // batches per group (cfg.pipeline_depth)
  uint32_t max_group_tiles = 0;
  uint32_t max_tasks = 0;
  uint32_t max_tiles = 0;
  uint32_t key_passes = 0;
  uint32_t key_bits = 0;
  uint64_t groups = 0;          // groups formed
  uint64_t launch_seq = 0;
  uint64_t* done_host = nullptr;     // pinned: [0] launch k-1 complete, written by launch k;
                                     // [1] the last launch whose retention stopped early
  uint64_t* done_dev = nullptr;
  std::vector<Staging> staging;   // host batches: a slot per batch of the forming group and of three in flight
  CopyPool* copy_pool = nullptr;  // host batches (created with the first one)

  // ---- tickets
  uint64_t last_ticket = 0;
  std::vector<uint32_t> ticket_n;        // [kStatsRing] records of each recent ticket (stats)
  // completion: tickets are applied in order, launch after launch. marks = {hi, L}: every ticket
  // <= hi not covered by an earlier mark is applied by launch L (empty tickets count with the
  // non-empty one before them); every ticket <= done_ticket is complete.
  std::deque<std::pair<uint64_t, uint64_t>> marks;
  uint64_t done_ticket = 0;

  // ---- host mirrors of control state
  std::vector<uint64_t> ring;  // [P] host copy of DevState::ring
  std::vector<uint64_t> key;   // [P] placement key of each partition (FORMAT.md §9 list order)
  std::vector<uint32_t> is_leader, leader_slot, ranks;  // ranks [P][RF]
  std::vector<uint64_t> term;
  // votes (Raft's votedFor per term, raft_meta): the term of the last vote, the candidate, and whether
  // this replica led that term (rmq_become_leader succeeded in it)
  std::vector<uint64_t> vterm;
  std::vector<uint32_t> vfor, vled;
  std::chrono::steady_clock::time_point place_time = std::chrono::steady_clock::now();  // last placement
  rmq::Replication* repl = nullptr;  // replication transport attached (collective mode)

  // ---- fetch: its own stream and scratch, serialised by fetch_mu (engine state under mu only while
  // the fetch is ordered against the pipeline stream)
  std::mutex fetch_mu;
  // fetches in flight (rmq_fetch_async), each with its own scratch: a fetch is ordered after the
  // launches issued before it and before the ones issued after it; the host only waits in
  // rmq_fetch_poll (or when every slot is taken: the oldest is completed into its caller's arrays
  // and its result kept for its poll)
  struct FetchSlot {
    uint32_t* d_req = nullptr;
    uint64_t* d_res = nullptr;
    uint64_t* d_aux = nullptr;
    uint32_t* d_cpre = nullptr;
    uint64_t* d_csum = nullptr;   // two halves of csum_lines lines: a fetch adds into one, its gather
                                  // zeroes the other for the next fetch of the slot (same stream)
    uint64_t* d_csum_fill = nullptr;  // csum_lines lines more: the chunk sums a filling call's fill kernel
                                      //   writes whole for its gather (RMQ_FETCH_FILL); made by the slot's
                                      //   first filling call
    uint32_t csum_lines = 0;
    uint32_t csum_par = 0;
    uint32_t* h_req = nullptr;   // pinned
    uint64_t* h_res = nullptr;   // pinned [cap][4] + {bytes needed, 0}
    uint32_t* h_bud = nullptr;   // pinned [cap] byte budgets of host rows (rmq_fetch_bytes), copied at the call
    uint32_t* d_bud = nullptr;   // [cap] their device copy where RMQ_FETCH_DMA moves the request rows
    uint64_t* h_at = nullptr;    // pinned [cap] explicit offsets of host rows (rmq_fetch_at), copied at the call;
                                 //   made by the slot's first call that passes offsets (as d_at)
    uint64_t* d_at = nullptr;    // [cap] their device copy where RMQ_FETCH_DMA moves the request rows
    // record table (rmq_fetch_table), made by the slot's first table call (as d_at and d_csum_fill)
    uint64_t* d_tsum = nullptr;  // csum_lines words: the table words of each chunk of rows
    uint64_t* d_trow = nullptr;  // [cap + 1] device staging of a host rec_row
    uint64_t* d_tpos = nullptr;  // [tpos_alloc] device staging of a host rec_pos (grows as d_out does)
    uint64_t tpos_alloc = 0;
    uint32_t cap = 0;
    uint8_t* d_out = nullptr;    // device staging of a host output
    uint64_t out_alloc = 0;
    hipEvent_t ev = nullptr;     // its kernels done (result rows and bytes needed in place)
    hipEvent_t ev_copy = nullptr;  // host output copies done
    hipEvent_t ev_in = nullptr;    // (DMA rows) request rows on the device
    hipEvent_t ev_k = nullptr;     // (DMA rows) kernels done: the result rows' copy may start
    bool rows_pinned = false;      // the caller's rows read / written in place (pinned or device rows)
    uint64_t* need = nullptr;      // bytes needed: a word of fetch_need_host (the gather stores it)
    uint64_t* need_dev = nullptr;  // its device address
    uint64_t* tneed = nullptr;     // table words needed (rec_row[n]): the slot's second word of fetch_need_host
    uint64_t* tneed_dev = nullptr;
    // the fetch in flight: ticket 0 = idle; phase 1: kernels, 2: host output copies
    uint64_t ticket = 0;
    int phase = 0;
    int rc = 0;
    uint32_t n = 0, mem = 0;
    uint8_t* out = nullptr;
    uint64_t out_cap = 0;
    rmq_fetch_res* res = nullptr;
    bool table = false;            // a ticket with a record table: rec_row[n] > t_cap completes RMQ_ENOSPC
    uint64_t* t_row = nullptr;     //   a host table's arrays (copied back with the host output), else null
    uint64_t* t_pos = nullptr;
    uint64_t t_cap = 0;
    bool pending = false;  // its kernels held back to go with the next asynchronous fetches (fetch_flush)
    FetchArgs args{};      //   and their arguments
  };
  static constexpr uint32_t kFetchSlots = 4;
  FetchSlot fslot[kFetchSlots];
  uint32_t fslot_next = 0;
  uint64_t* fetch_need_host = nullptr;  // [2][kFetchSlots] coherent pinned words (FetchSlot::need, then ::tneed)
  uint64_t fetch_seq = 0;        // tickets
  std::vector<uint32_t> fetch_stamp;  // RMQ_FETCH_COMMIT duplicate check ([P][C] generation stamps)
  std::vector<uint32_t> fetch_stamp_rep;  // the same for replica reads ([P]: one replica cursor each)
  uint32_t fetch_gen = 0;
  std::deque<std::array<uint64_t, 3>> fetch_done;  // {ticket, rc, bytes used} completed, not yet polled
  std::vector<uint32_t> fpend;  // slots of asynchronous fetches whose kernels wait for fetch_flush (under mu)

  // ---- rmq_lag (lag.cpp): calls serialised by lag_mu (taken before mu); the page-locked staging of
  // host rows, grown on demand, and the event behind the call's kernel
  std::mutex lag_mu;
  struct Lag {
    rmq_fetch_req* h_req = nullptr;  // [cap]
    uint64_t* h_at = nullptr;        // [cap] explicit offsets
    rmq_lag_res* h_res = nullptr;    // [cap]
    uint32_t cap = 0;
    hipEvent_t ev = nullptr;
  } lag;

  // ---- rmq_unpack (unpack.cpp): calls serialised by unpack_mu (taken before mu); the page-locked
  // staging of host rows and their device copy, the chunk-sum scratch, the control words on both
  // sides, all grown on demand, and the event behind the call's last copy
  std::mutex unpack_mu;
  struct Unpack {
    rmq_fetch_res* h_rows = nullptr;  // [row_cap] page-locked
    uint64_t* d_rows = nullptr;       // [row_cap][4]
    uint64_t* d_rsum = nullptr;       // [row_cap / kFetchChunk + 1]
    uint32_t row_cap = 0;
    uint64_t* d_lsum = nullptr;       // [lsum_cap]
    uint64_t lsum_cap = 0;
    uint64_t* h_ctl = nullptr;        // [kUnpackCtlWords] page-locked
    uint64_t* d_ctl = nullptr;        // [kUnpackCtlWords]
    hipEvent_t ev = nullptr;
  } unpack;

  // ---- consumer commits: staging slots (pinned items -> device by one copy on the pipeline
  // stream), so a commit is ordered with the append stream without waiting for it
  struct CommitSlot {
    uint8_t* h = nullptr;
    uint8_t* d = nullptr;
    uint32_t cap = 0;
    hipEvent_t ev = nullptr;
    bool used = false;
  };
  // a slot is reused once the commit that last used it has run on the pipeline stream, which may
  // queue a few launches ahead of it (RMQ_AHEAD): enough slots that a commit rarely waits
  static constexpr uint32_t kCommitSlots = 16;
  CommitSlot cslot[kCommitSlots];
  uint32_t cslot_next = 0;
  std::vector<uint32_t> lww_stamp;  // [P * C] generation of the last commit item seen per slot
  uint32_t lww_gen = 0;
  // consumer-offset tickets (rmq_commit_consumer_offset): the row version of every partition (host
  // mirror of DevState::cver) and, per pending ticket, the (partition, version) pairs it waits for
  std::vector<uint64_t> cver;
  std::vector<uint32_t> cstamp;  // [P] generation of the last call that bumped the version
  uint32_t cstamp_gen = 0;
  uint64_t off_ticket_seq = 0;
  std::deque<std::pair<uint64_t, std::vector<std::pair<uint32_t, uint64_t>>>> off_tickets;
  static constexpr size_t kMaxOffsetTickets = 256;   // the newest unpolled ones are kept

  // ---- profile: pipeline launches are timed as one region (event before the first launch after
  // enable, event at the next drain) so no per-launch events sit between kernels; fetch kernels
  // keep per-launch event pairs (prof[3], prof[4]), and so do every rmq_scrub (prof[2]), every rmq_repair (prof[5]), every rmq_repair_remote (prof[6]), every rmq_restore (prof[7]), every rmq_reindex (prof[8]), every fetch's record-table kernels (prof[9]), every rmq_lag (prof[10]) and every rmq_unpack (prof[11])
  uint32_t profile = 0;
  uint32_t fetch_replay = 1;     // rmq_profile_enable(k >= 2): each fetch's kernels run k times
  uint64_t prof_fetch_runs = 0;
  struct ProfRegion {
    uint64_t launches = 0, batches = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    bool started = false, ended = false;
  } region;
  std::vector<EvPair> prof[12];

  // ---- per-subsystem scratch, grown on demand and freed by its subsystem
  // ack scratch (offsets.cpp)
  uint32_t* d_ctl32 = nullptr;
  uint64_t* d_ctl64 = nullptr;
  uint32_t ctl_cap = 0;
  uint64_t* state_stage = nullptr;  // page-locked staging of rmq_get_partition_states
  size_t state_stage_words = 0;
  // rmq_scrub, rmq_repair, rmq_repair_remote, rmq_reindex (audit.cpp): device buffers of one call's
  // range of n partitions, grown on demand (a capacity in elements next to each)
  struct Audit {
    uint64_t* tbase = nullptr;    // [n + 1] the plan's scan
    uint64_t* rows = nullptr;     // [n][4] the result rows
    uint8_t* verdict = nullptr;   // [tasks of the bound] the first pass's verdicts
    uint64_t* counts = nullptr;   // [n][3] the repair's counters
    uint64_t* gaps = nullptr;     // [tasks][2] rmq_reindex: the gap list
    uint64_t* scratch = nullptr;  // [tasks][2] rmq_reindex: the rebuilt entries
    uint64_t* rcounts = nullptr;  // [n][3] rmq_reindex's counters, then the gap counter's word
    uint64_t tbase_cap = 0, rows_cap = 0, verdict_cap = 0, counts_cap = 0, gaps_cap = 0, scratch_cap = 0,
             rcounts_cap = 0;
  } au;
  // rmq_repair_remote (repair_remote.cpp): device buffers grown on demand (a capacity next to each),
  // fixed control words with their page-locked mirror, the per-destination budget and the fault hook
  struct RemoteRepair {
    uint8_t* want = nullptr;     // [tasks] RemoteReqArgs::want
    uint64_t* fetched = nullptr; // [n][2]
    uint32_t* cand = nullptr;    // [n][RF - 1]
    uint64_t* pkey = nullptr;    // [P]
    RemoteKey* keys = nullptr;   // [P]
    uint8_t* lists = nullptr;    // request lists, one per destination
    uint8_t* rin = nullptr;      // request lists received
    uint64_t* sv = nullptr;      // [requests received]
    uint8_t* out = nullptr;      // responses
    uint8_t* in = nullptr;       // responses received
    uint64_t want_cap = 0, fetched_cap = 0, cand_cap = 0, key_cap = 0, lists_cap = 0, rin_cap = 0, sv_cap = 0,
             out_cap = 0, in_cap = 0;
    uint64_t* csum = nullptr;    // [kMaxWorld][kRemoteChunks]
    uint64_t* words = nullptr;   // [kRemoteWords] exchanged words, counters and totals
    uint64_t* h_words = nullptr; // pinned mirror, then the list headers
    hipEvent_t ev = nullptr;
    DevRecord dev;               // every device buffer above, noted where repair_remote.cpp makes it
    bool flip[kMaxWorld] = {};   // rmq_fault_corrupt_repair: the next response to q
    int64_t flip_at[kMaxWorld] = {};
  } rr;
  // rmq_restore: device scratch grown on demand (a host buffer's runs, the table words, the checked
  // items with their record scan and verdict keys)
  struct Restore {
    uint8_t* buf = nullptr;
    uint64_t* tab = nullptr;
    RestoreItem* items = nullptr;
    uint64_t* rbase = nullptr;   // [items + 1]
    uint64_t* key = nullptr;     // [items]
    uint64_t buf_cap = 0, tab_cap = 0, items_cap = 0;
  } rs;

  // ---- diagnostics: RMQ_STAMPS=<csv> records per-wave phase stamps of launch RMQ_STAMPS_AT (default 100)
  const char* stamps_path = nullptr;
  uint64_t* d_stamps = nullptr;
  rmq::RolePlan stamps_plan;  // the roles of the stamped launch
};

namespace rmq {

inline int hip_fail(hipError_t e) {
  if (e == hipSuccess) return RMQ_OK;
  std::fprintf(stderr, "ripplemq: HIP error %d (%s)\n", (int)e, hipGetErrorString(e));
  return e == hipErrorOutOfMemory ? RMQ_ENOMEM : RMQ_EDEVICE;
}

#define HIP_TRY(x)                      \
  do {                                  \
    hipError_t _e = (x);                \
    if (_e != hipSuccess) return hip_fail(_e); \
  } while (0)

template <typename T>
int dalloc(T** p, size_t count) {
  *p = nullptr;
  if (!count) count = 1;
  HIP_TRY(hipMalloc((void**)p, count * sizeof(T)));
  // The null stream does not order with the engine's non-blocking streams: finish the zeroing
  // before any engine stream can touch the buffer (a lazily allocated staging buffer would
  // otherwise be zeroed after its first H2D copy).
  HIP_TRY(hipMemset(*p, 0, count * sizeof(T)));
  HIP_TRY(hipDeviceSynchronize());
  return RMQ_OK;
}

// Grow a device buffer on demand (never shrunk) through dalloc: the fresh buffer zeroed and the device
// synchronised, dalloc's code with the pointer null and the capacity 0 on failure.
template <typename T>
int grow(T** p, uint64_t* cap, uint64_t need) {
  if (*cap >= need && *p) return RMQ_OK;
  if (*p) hipFree(*p);
  *p = nullptr;
  *cap = 0;
  int rc = dalloc(p, (size_t)need);
  if (rc) return rc;
  *cap = need;
  return RMQ_OK;
}

// Memory that lives as long as the engine: recorded where it is allocated, freed by free_engine from
// the lists alone (a buffer whose zeroing failed is recorded too).
template <typename T>
int owned_dalloc(rmq_engine* e, T** p, size_t count) {
  const int rc = dalloc(p, count);
  if (*p) e->owned_dev.push_back(*p);
  return rc;
}
template <typename T>
int owned_host_alloc(rmq_engine* e, T** p, size_t bytes, unsigned flags) {
  *p = nullptr;
  HIP_TRY(hipHostMalloc((void**)p, bytes, flags));
  e->owned_host.push_back(*p);
  return RMQ_OK;
}

// rmq_restore's grow, which stages asynchronously right after it: no zeroing, no device-wide
// synchronise, and every failure is RMQ_ENOMEM with the HIP error cleared and the old buffer gone.
template <typename T>
int restore_grow(T** p, uint64_t* cap, uint64_t need) {
  if (*cap >= need && *p) return RMQ_OK;
  if (*p) hipFree(*p);
  *p = nullptr;
  *cap = 0;
  if (hipMalloc((void**)p, (size_t)need * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return RMQ_ENOMEM;
  }
  *cap = need;
  return RMQ_OK;
}

// Synchronous typed copies between the host and device state: n words, or a whole host vector.
template <typename T>
int read_words(T* dst, const T* src, size_t n = 1) {
  HIP_TRY(hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost));
  return RMQ_OK;
}
template <typename T>
int write_words(T* dst, const T* src, size_t n = 1) {
  HIP_TRY(hipMemcpy(dst, src, n * sizeof(T), hipMemcpyHostToDevice));
  return RMQ_OK;
}
template <typename T>
int read_words(std::vector<T>& h, const T* d) { return read_words(h.data(), d, h.size()); }
template <typename T>
int write_words(T* d, const std::vector<T>& h) { return write_words(d, h.data(), h.size()); }

// A ring descriptor (DevState::ring) taken apart on the host, next to kernels.hpp's ring_ref.
inline uint64_t ring_bytes(uint64_t desc) { return 1ull << (desc & 63ull); }
inline RingRef ring_of(const rmq_engine* e, uint32_t p) {
  return ring_ref(e->ring[p], e->st.interval_log2, e->st.icap_mul);
}
inline void release_ring(rmq_engine* e, uint64_t desc) { e->pool.release((uint32_t)(desc & 63ull), desc & ~63ull); }

// The placement's host mirror: the replica slots of partition p this rank holds (bit r: slot r, as
// DevState::local_mask), whether it holds any, and the rank the placement names leader.
inline uint32_t local_slots(const rmq_engine* e, uint32_t p) {
  uint32_t mask = 0;
  for (uint32_t r = 0; r < e->cfg.replication_factor; ++r)
    mask |= (e->ranks[(size_t)p * e->cfg.replication_factor + r] == e->cfg.rank ? 1u : 0u) << r;
  return mask;
}
inline bool is_local(const rmq_engine* e, uint32_t p) { return local_slots(e, p) != 0; }
inline uint32_t leader_rank(const rmq_engine* e, uint32_t p) {
  return e->ranks[(size_t)p * e->cfg.replication_factor + e->leader_slot[p]];
}

// The prologue of a call under the engine lock: this thread's device, then the pipeline as far as the
// call needs it (drain, quiesce, settle or a wait of the caller's).
inline int begin_call(rmq_engine* e, int (*wait)(rmq_engine*)) {
  HIP_TRY(hipSetDevice(e->device));
  return wait(e);
}

// engine.cpp
bool is_pow2(uint64_t v);
uint32_t ilog2(uint64_t v);
int equalize_state_sets(rmq_engine* e);  // both state sets hold every log end (drained; before a role changes)
int check_err(rmq_engine* e);
int event_wait(hipEvent_t ev);  // spin on queries (20 ms), then block
int stream_wait(hipStream_t s);  // the same for everything issued on a stream
hipEvent_t pool_event(rmq_engine* e);
// append.cpp
int flush(rmq_engine* e);
int drain(rmq_engine* e);
int quiesce(rmq_engine* e);
int settle(rmq_engine* e);  // drain, or with a transport (where a flush is collective) quiesce
int late_retention(rmq_engine* e);  // the last applied group's retention, where its own launch stopped early
void dump_stamps(rmq_engine* e);    // RMQ_STAMPS: the stamped launch's phase stamps, at destruction
void staging_free(rmq_engine* e);
// offsets.cpp
int poll_offsets(rmq_engine* e, uint64_t ticket);  // rmq_poll_commit of a consumer-offset ticket (device set)
void offsets_free(rmq_engine* e);
// fetch.cpp
int fetch_flush(rmq_engine* e);  // launch the asynchronous fetches held back (under mu)
void fetch_free(rmq_engine* e);
// lag.cpp
void lag_free(rmq_engine* e);  // the staging of host rows (its event goes with the engine)
// unpack.cpp
void unpack_free(rmq_engine* e);  // rmq_unpack's staging, scratch and event
// The engine lock of every call: held-back asynchronous fetches go to the pipeline stream first, so
// whatever the call issues is ordered after them (their contract); a launch error stays sticky on the
// stream and surfaces at the next check.
struct EngineLock {
  std::lock_guard<std::mutex> g;
  explicit EngineLock(rmq_engine* e) : g(e->mu) {
    if (!e->fpend.empty() && hipSetDevice(e->device) == hipSuccess) (void)fetch_flush(e);
  }
};
// Workgroups of the audit kernels (the scrub's verify, the fetch verify): 8 per CU, or at most
// RMQ_AUDIT_WGS of them.
inline uint32_t audit_wgs(const rmq_engine* e) {
  const uint32_t wgs = std::max<uint32_t>(e->cu_count, 1u) * 8u;
  return e->knob.audit_wgs ? std::min(wgs, e->knob.audit_wgs) : wgs;
}
// audit.cpp
void audit_free(rmq_engine* e);
// replication.cpp
int repl_attach(rmq_engine* e, Transport* t);
void repl_free(rmq_engine* e);
int repl_set_lists(rmq_engine* e);
void repl_pipe_args(rmq_engine* e, PipeArgs& a, const GroupFlight* s2, const GroupFlight* s3);
int repl_before_launch(rmq_engine* e, PipeArgs& a);
int repl_after_launch(rmq_engine* e, const GroupFlight* s2, const GroupFlight* s3);
int repl_drain(rmq_engine* e);
int reset_catchup(rmq_engine* e);
// repair_remote.cpp
// The rounds of rmq_repair_remote (FORMAT.md §10 "Remote repair") after the first pass, engine
// drained, transport attached. a: the first pass's plan and verdicts with something still failing,
// or null (nothing to ask for: this rank only serves); wgs: the request kernel's grid;
// tasks: the verdicts' capacity; fetched: [n][2] host {pairs, bytes} (a != null); served: [2].
int repair_remote_rounds(rmq_engine* e, const RepairArgs* a, uint32_t wgs, uint64_t tasks, uint64_t* fetched,
                         uint64_t* served);
void repair_remote_free(rmq_engine* e);

}  // namespace rmq
