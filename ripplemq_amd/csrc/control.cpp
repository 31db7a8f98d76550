// control.cpp — the calls of the C-ABI that change a partition's role or ring: rmq_set_replicas,
// rmq_set_placement, rmq_become_leader, rmq_vote, rmq_set_vote, rmq_leader_silent, rmq_set_segments
// and rmq_set_replica_cursor (FORMAT.md §2, §6, §9).
//
// They are rare next to the append stream and run synchronously: each takes the engine lock, validates
// everything before it changes anything, settles the pipeline as far as it needs (begin_call), then
// reads and writes a few words of device state next to the host mirrors. The rules they share (who is
// local, what a leader that steps down does) are the file-local steps below.
#include "engine_internal.hpp"

using namespace rmq;

namespace {

// These partitions stop being led here: a former leader knows its own commit as the leader's
// (FORMAT.md §9 v4), and is_leader goes to 0 on the host and the device. One span of words from the
// lowest to the highest of them, whatever their number. The caller has equalized the state sets.
int step_down(rmq_engine* e, const std::vector<uint32_t>& ps) {
  if (ps.empty()) return RMQ_OK;
  const auto ends = std::minmax_element(ps.begin(), ps.end());
  const uint32_t lo = *ends.first;
  std::vector<uint64_t> c(*ends.second - lo + 1), lc(c.size());
  int rc = read_words(c, e->st.commit + lo);
  if (!rc) rc = read_words(lc, e->st.lcommit + lo);
  if (rc) return rc;
  for (uint32_t p : ps) {
    lc[p - lo] = std::max(lc[p - lo], c[p - lo]);
    e->is_leader[p] = 0;
  }
  rc = write_words(e->st.lcommit + lo, lc);
  return rc ? rc : write_words(e->st.is_leader + lo, &e->is_leader[lo], c.size());
}

// Placement of n partitions (engine locked). With a replication transport this is collective:
// every rank recomputes its out / in lists and checks them against its peers'.
int set_placement(rmq_engine* e, uint32_t n, const uint32_t* pidx, const uint64_t* key, const uint32_t* ranks,
                  const uint32_t* leader_slot) {
  const uint32_t P = e->cfg.num_partitions, RF = e->cfg.replication_factor;
  if (n && (!pidx || !ranks || !leader_slot)) return RMQ_EINVAL;
  for (uint32_t i = 0; i < n; ++i) {
    if (pidx[i] >= P) return RMQ_ENOPART;
    if (leader_slot[i] >= RF) return RMQ_EINVAL;
  }
  int rc = begin_call(e, drain);
  if (!rc) rc = equalize_state_sets(e);
  if (rc) return rc;
  // a placement keeps or ends this replica's leadership; it never starts one: a replica the
  // placement names leader leads once rmq_become_leader passes Raft's checks
  std::vector<uint32_t> demoted;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t p = pidx[i];
    std::copy_n(ranks + (size_t)i * RF, RF, &e->ranks[(size_t)p * RF]);
    e->leader_slot[p] = leader_slot[i];
    if (key) e->key[p] = key[i];
    if (e->is_leader[p] && leader_rank(e, p) != e->cfg.rank) demoted.push_back(p);
  }
  rc = step_down(e, demoted);
  std::vector<uint32_t> mask(P);
  for (uint32_t p = 0; p < P; ++p) mask[p] = local_slots(e, p);
  if (!rc) rc = write_words(e->st.local_mask, mask);
  if (!rc && n) {  // the election timer of every placed partition restarts
    std::vector<uint64_t> hd(P);
    rc = read_words(hd, e->st.heard);
    for (uint32_t i = 0; i < n; ++i) hd[pidx[i]] = e->repl ? e->repl->stamp : 0ull;
    if (!rc) rc = write_words(e->st.heard, hd);
    if (!rc) e->place_time = std::chrono::steady_clock::now();
  }
  if (rc) return rc;
  return e->repl ? repl_set_lists(e) : RMQ_OK;
}

// Before a vote reads a partition's term and log: without a transport every batch submitted is
// applied first (drain); with one, a flush would be collective (rmq_sync), so only what is issued is
// waited for: the pipeline stream and the rounds' ingest on the exchange stream.
int vote_settle(rmq_engine* e) {
  if (!e->repl) return drain(e);
  int rc = quiesce(e);
  return rc ? rc : hip_fail(hipStreamSynchronize(e->repl->xchg_s));
}

// rmq_set_segments, step 1: every item before anything moves.
int segments_validate(const rmq_engine* e, uint32_t n, const uint32_t* pidx, const uint64_t* seg) {
  const uint32_t P = e->cfg.num_partitions;
  std::vector<uint8_t> seen(P, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (pidx[i] >= P) return RMQ_ENOPART;
    if (seen[pidx[i]]++ || !is_pow2(seg[i]) || seg[i] < 4ull * e->cfg.index_interval || seg[i] > e->st.rstride)
      return RMQ_EINVAL;
  }
  return RMQ_OK;
}

// The new rings of a move that does not happen go back to the pool; rc passes through.
int segments_rollback(rmq_engine* e, const std::vector<MigrateItem>& items, int rc) {
  for (const MigrateItem& it : items) release_ring(e, it.new_desc);
  return rc;
}

// Step 2: a new ring for every partition whose size changes, all or nothing.
int segments_alloc(rmq_engine* e, uint32_t n, const uint32_t* pidx, const uint64_t* seg,
                   std::vector<MigrateItem>& items) {
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t p = pidx[i], lg = ilog2(seg[i]);
    if (ring_bytes(e->ring[p]) == seg[i]) continue;
    uint64_t off = 0;
    if (!e->pool.alloc(lg, &off)) return segments_rollback(e, items, RMQ_ENOMEM);
    MigrateItem it{};
    it.p = p;
    it.old_desc = e->ring[p];
    it.new_desc = off | lg;
    items.push_back(it);
  }
  return RMQ_OK;
}

// Step 3: the retained range of every moved partition; a shrinking ring first applies retention at its
// new size (FORMAT.md §4: start = the first record at or after used - S', from the index).
int segments_retained(rmq_engine* e, std::vector<MigrateItem>& items) {
  const uint32_t P = e->cfg.num_partitions, ilog = e->st.interval_log2;
  std::vector<uint64_t> spos(P), soff(P), used(P);
  int rc = read_words(spos, e->st.start_pos);
  if (!rc) rc = read_words(soff, e->st.start_off);
  if (!rc) rc = read_words(used, e->st.used);
  for (MigrateItem& it : items) {
    if (rc) return rc;
    const uint64_t S1 = ring_bytes(it.new_desc);
    it.spos = spos[it.p];
    it.soff = soff[it.p];
    it.used = used[it.p];
    if (it.used - it.spos <= S1) continue;
    const uint64_t m = (it.used - S1 + (1ull << ilog) - 1) >> ilog;
    const RingRef o = ring_ref(it.old_desc, ilog, e->st.icap_mul);
    uint64_t ent[2];
    rc = read_words(ent, e->st.index + (o.ibase + m % o.icap) * 2, 2);
    it.soff = ent[0];
    it.spos = ent[1];
  }
  return rc;
}

// Step 4: the workgroups of each move, its new ring in kMigrateChunk pieces; returns their number.
uint32_t segments_chunks(std::vector<MigrateItem>& items) {
  uint32_t chunks = 0;
  for (MigrateItem& it : items) {
    it.chunk0 = chunks;
    chunks += (uint32_t)((ring_bytes(it.new_desc) + kMigrateChunk - 1) / kMigrateChunk);
  }
  return chunks;
}

// Step 5: launch the moves; then the new rings are the partitions' and the old ones go back to the
// pool, or nothing was launched and the new ones go back.
int segments_move(rmq_engine* e, const std::vector<MigrateItem>& items, uint32_t chunks) {
  MigrateItem* d_items = nullptr;
  int rc = dalloc(&d_items, items.size());
  if (!rc) rc = write_words(d_items, items.data(), items.size());
  if (!rc) {
    launch_migrate(e->st, d_items, (uint32_t)items.size(), chunks, e->main_s);
    if (hipGetLastError() != hipSuccess) rc = RMQ_EDEVICE;
  }
  if (rc) {
    segments_rollback(e, items, rc);
  } else {
    for (const MigrateItem& it : items) {
      e->ring[it.p] = it.new_desc;
      release_ring(e, it.old_desc);
    }
    rc = hip_fail(hipStreamSynchronize(e->main_s));
    if (!rc) rc = check_err(e);
  }
  if (d_items) hipFree(d_items);
  return rc;
}

}  // namespace

extern "C" {

int rmq_set_replicas(rmq_engine* e, uint32_t pidx, const uint32_t* ranks, uint32_t rf, uint32_t leader_slot) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  if (pidx >= e->cfg.num_partitions) return RMQ_ENOPART;
  if (!ranks || rf != e->cfg.replication_factor || leader_slot >= rf) return RMQ_EINVAL;
  return set_placement(e, 1, &pidx, nullptr, ranks, &leader_slot);
}

int rmq_set_placement(rmq_engine* e, uint32_t n, const uint32_t* pidx, const uint64_t* key, const uint32_t* ranks,
                      const uint32_t* leader_slot) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  return set_placement(e, n, pidx, key, ranks, leader_slot);
}

int rmq_become_leader(rmq_engine* e, uint32_t pidx, uint64_t term) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  const uint32_t P = e->cfg.num_partitions;
  if (pidx != RMQ_ALL_PARTITIONS && pidx >= P) return RMQ_ENOPART;
  const uint32_t lo = pidx == RMQ_ALL_PARTITIONS ? 0 : pidx, hi = pidx == RMQ_ALL_PARTITIONS ? P : pidx + 1;
  const size_t m = hi - lo;
  for (uint32_t p = lo; p < hi; ++p) {  // validate everything before changing anything
    if (!is_local(e, p)) return RMQ_EINVAL;
    // with a transport the placement (collective) names the leader; this starts its term
    if (e->repl && leader_rank(e, p) != e->cfg.rank) return RMQ_EINVAL;
  }
  int rc = begin_call(e, drain);
  if (!rc) rc = equalize_state_sets(e);
  // a follower adopts newer leader terms from replication rounds (FORMAT.md §9): the device holds
  // the current terms
  if (!rc) rc = read_words(&e->term[lo], e->st.term + lo, m);
  if (rc) return rc;
  for (uint32_t p = lo; p < hi; ++p) {
    if (term < e->term[p]) return RMQ_EINVAL;
    // one leader per term: not a term this replica led, nor one it gave its vote to another candidate
    if (e->vterm[p] == term && (e->vled[p] || e->vfor[p] != e->cfg.rank)) return RMQ_ETERM;
  }
  // Raft's vote restriction, as far as this replica can tell: it may not lead a partition whose
  // leader committed records its log does not verifiably hold (leader_commit from rounds and
  // commit notices; verified: the whole log when it was matched in the current term, else the
  // replica's own commit)
  std::vector<uint64_t> leo(m), lc(m), mt(m), cm(m);
  rc = read_words(leo, e->st.leo + lo);
  if (!rc) rc = read_words(lc, e->st.lcommit + lo);
  if (!rc) rc = read_words(mt, e->st.mterm + lo);
  if (!rc) rc = read_words(cm, e->st.commit + lo);
  if (rc) return rc;
  for (size_t i = 0; i < m; ++i)
    if ((mt[i] == e->term[lo + i] ? leo[i] : cm[i]) < lc[i]) return RMQ_ESTALE;  // (always led here: lc = 0)
  for (uint32_t p = lo; p < hi; ++p) {
    // without a transport the first local slot leads; with one, the placed slot
    if (!e->repl) e->leader_slot[p] = (uint32_t)__builtin_ctz(local_slots(e, p));
    e->is_leader[p] = 1;
    e->term[p] = term;
    e->vterm[p] = term;  // a leader's vote is its own
    e->vfor[p] = e->cfg.rank;
    e->vled[p] = 1;
  }
  rc = write_words(e->st.is_leader + lo, &e->is_leader[lo], m);
  if (!rc) rc = write_words(e->st.term + lo, &e->term[lo], m);
  if (rc) return rc;
  launch_become_leader(e->st, pidx, e->main_s);
  HIP_TRY(hipGetLastError());
  rc = drain(e);
  // Raft's leader start: nextIndex of every follower = the leader's last index + 1
  if (!rc && e->repl) rc = reset_catchup(e);
  return rc;
}

int rmq_vote(rmq_engine* e, uint32_t pidx, uint64_t term, uint32_t candidate, uint64_t cand_last_log_term,
             uint64_t cand_log_end, uint32_t* granted) {
  if (!e || !granted) return RMQ_EINVAL;
  *granted = 0;
  EngineLock g(e);
  if (pidx >= e->cfg.num_partitions) return RMQ_ENOPART;
  int rc = begin_call(e, vote_settle);
  if (rc) return rc;
  // with a transport nothing is flushed (a flush is collective): a leader of pidx whose groups in
  // flight may still add its records answers RMQ_PENDING and changes nothing (a delayed RequestVote)
  if (e->repl && e->is_leader[pidx] && (e->forming.nb || e->has1 || e->has2)) return RMQ_PENDING;
  uint64_t cur = 0, lterm = 0, leo = 0;
  rc = read_words(&cur, e->st.term + pidx);
  if (!rc) rc = read_words(&lterm, e->st.lterm + pidx);
  if (!rc) rc = read_words(&leo, e->st.leo + pidx);
  if (rc) return rc;
  lterm &= ~kLtermBound;  // an unknown last log term: its upper bound (a stricter vote)
  if (term < cur) return RMQ_OK;  // a candidate of an older term
  if (term > cur) {  // Raft: a newer term is adopted; a leader steps down
    e->term[pidx] = term;
    rc = write_words(e->st.term + pidx, &term);
    if (!rc && e->is_leader[pidx]) {
      rc = equalize_state_sets(e);
      if (!rc) rc = step_down(e, {pidx});
    }
    if (rc) return rc;
  }
  const bool up = cand_last_log_term > lterm || (cand_last_log_term == lterm && cand_log_end >= leo);
  const bool free_vote = e->vterm[pidx] != term || (!e->vled[pidx] && e->vfor[pidx] == candidate);
  if (up && free_vote) {
    e->vterm[pidx] = term;
    e->vfor[pidx] = candidate;
    e->vled[pidx] = 0;
    *granted = 1;
  }
  return RMQ_OK;
}

int rmq_set_vote(rmq_engine* e, uint32_t pidx, uint64_t term, uint32_t voted_for) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  if (pidx >= e->cfg.num_partitions) return RMQ_ENOPART;
  int rc = begin_call(e, vote_settle);
  uint64_t cur = 0;
  if (!rc) rc = read_words(&cur, e->st.term + pidx);
  if (!rc && term > cur) {
    e->term[pidx] = term;
    rc = write_words(e->st.term + pidx, &term);
  }
  if (rc) return rc;
  e->vterm[pidx] = term;
  e->vfor[pidx] = voted_for;
  e->vled[pidx] = 0;
  return RMQ_OK;
}

int rmq_leader_silent(rmq_engine* e, uint32_t silent_rounds, uint32_t timeout_ms, uint32_t* out_pidx, uint32_t cap,
                      uint32_t* n) {
  if (!e || !n || (cap && !out_pidx)) return RMQ_EINVAL;
  *n = 0;
  EngineLock g(e);
  const uint32_t P = e->cfg.num_partitions;
  HIP_TRY(hipSetDevice(e->device));
  if (e->repl) HIP_TRY(hipStreamSynchronize(e->repl->xchg_s));  // (the rounds' ingest writes the words)
  std::vector<uint64_t> hd(P);
  int rc = read_words(hd, e->st.heard);
  if (rc) return rc;
  const uint64_t cur = e->repl ? e->repl->stamp : 0ull;
  const auto now = std::chrono::steady_clock::now();
  uint32_t k = 0;
  for (uint32_t p = 0; p < P; ++p) {
    if (e->is_leader[p] || !is_local(e, p) || hd[p] + silent_rounds > cur) continue;
    // wall time since the leader was last heard (the round's posting, or the placement)
    auto at = e->place_time;
    if (e->repl && hd[p] && cur - hd[p] < 64) at = std::max(at, e->repl->stamp_time[hd[p] % 64]);
    if (std::chrono::duration_cast<std::chrono::milliseconds>(now - at).count() < (long long)timeout_ms) continue;
    if (k < cap) out_pidx[k] = p;
    ++k;
  }
  *n = k;
  return RMQ_OK;
}

// The steps above, in their order (fetches run on the pipeline stream: the drain waits for them too).
int rmq_set_segments(rmq_engine* e, uint32_t n, const uint32_t* pidx, const uint64_t* seg) {
  if (!e) return RMQ_EINVAL;
  if (!n) return RMQ_OK;
  if (!pidx || !seg) return RMQ_EINVAL;
  std::lock_guard<std::mutex> fg(e->fetch_mu);  // no fetch reads a ring while it moves
  EngineLock g(e);
  int rc = segments_validate(e, n, pidx, seg);
  if (!rc) rc = begin_call(e, drain);
  std::vector<MigrateItem> items;
  if (!rc) rc = segments_alloc(e, n, pidx, seg, items);
  if (rc || items.empty()) return rc;
  rc = segments_retained(e, items);
  return rc ? segments_rollback(e, items, rc) : segments_move(e, items, segments_chunks(items));
}

int rmq_set_replica_cursor(rmq_engine* e, uint32_t n, const uint32_t* pidx, const uint64_t* offset) {
  if (!e || (n && (!pidx || !offset))) return RMQ_EINVAL;
  EngineLock g(e);
  const uint32_t P = e->cfg.num_partitions;
  for (uint32_t i = 0; i < n; ++i)
    if (pidx[i] >= P) return RMQ_ENOPART;
  if (!n) return RMQ_OK;
  int rc = begin_call(e, quiesce);  // (fetches on the pipeline stream read and commit the cursors)
  std::vector<uint64_t> cur(P);
  if (!rc) rc = read_words(cur, e->st.rcur);
  for (uint32_t i = 0; i < n; ++i) cur[pidx[i]] = offset[i];
  return rc ? rc : write_words(e->st.rcur, cur);
}

}  // extern "C"
