// repl_plan.hpp — the arithmetic of the replication protocol's host side (FORMAT.md §9): the out / in
// lists of a placement, the round buffers' bounds, and where one round's regions and verify tasks lie.
// Pure functions of integers. Plain C++ with no device header (the constants of kernels.hpp come in
// as arguments), so that it also builds into a stand-alone program under the sanitizers
// (tools/repl_plan_main.cpp). replication.cpp and repair_remote.cpp only turn the results into
// pointers, uploads and exchanges.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace rmq {

constexpr uint32_t kPlanMaxWorld = 16;  // kMaxWorld of kernels.hpp (engine_internal.hpp asserts it)

// Regions and lists packed one after the other start on 16 bytes.
inline uint64_t pad16(uint64_t n) { return (n + 15) & ~15ull; }

// ---- lists from a placement

struct Placement {
  uint32_t P = 0, RF = 0, W = 0, me = 0;
  const uint32_t* ranks = nullptr;        // [P][RF]
  const uint32_t* leader_slot = nullptr;  // [P]
  const uint64_t* key = nullptr;          // [P]
};

// out list: (led partition, remote slot) grouped by destination, ascending (key, slot);
// in list: (followed partition, local slot) grouped by source, the same order on both sides
struct ReplLists {
  std::vector<uint32_t> xo_p, xo_slot, xo_start;  // xo_start [W + 1]
  std::vector<uint32_t> xi_p, xi_slot, xi_start;  // xi_start [W + 1]
  std::vector<uint64_t> keysum, keysum_in;        // [W] sums of entry_hash over each destination / source
  std::vector<uint32_t> outidx;                   // [P][RF] index in the out list, ~0: not a remote slot led here
  uint32_t max_remote = 0;                        // most remote slots of one led partition
  bool bad = false;  // a row names a rank >= W, or a led partition has more than max_remote_slots remote slots
};

inline uint64_t entry_hash(uint64_t key, uint32_t slot, uint32_t max_rf) { return key * max_rf + slot; }

inline ReplLists plan_lists(const Placement& pl, uint32_t max_remote_slots, uint32_t max_rf) {
  struct Entry {
    uint64_t key;
    uint32_t slot, p;
    bool operator<(const Entry& o) const { return key != o.key ? key < o.key : slot < o.slot; }
  };
  const uint32_t P = pl.P, RF = pl.RF, W = pl.W, me = pl.me;
  std::vector<std::vector<Entry>> out(W), in(W);
  ReplLists l;
  for (uint32_t p = 0; p < P; ++p) {
    const uint32_t* rk = &pl.ranks[(size_t)p * RF];
    const uint32_t lead = rk[pl.leader_slot[p]];
    uint32_t remote = 0;
    for (uint32_t s = 0; s < RF; ++s) {
      if (rk[s] >= W) l.bad = true;
      else if (lead == me && rk[s] != me) {
        out[rk[s]].push_back({pl.key[p], s, p});
        ++remote;
      } else if (lead != me && rk[s] == me && lead < W) {
        in[lead].push_back({pl.key[p], s, p});
      }
    }
    if (remote > max_remote_slots) l.bad = true;
  }
  l.xo_start.assign(W + 1, 0);
  l.xi_start.assign(W + 1, 0);
  l.keysum.assign(W, 0);
  l.keysum_in.assign(W, 0);
  l.outidx.assign((size_t)P * RF, ~0u);
  for (uint32_t q = 0; q < W; ++q) {
    std::sort(out[q].begin(), out[q].end());
    std::sort(in[q].begin(), in[q].end());
    l.xo_start[q] = (uint32_t)l.xo_p.size();
    for (const Entry& x : out[q]) {
      l.outidx[(size_t)x.p * RF + x.slot] = (uint32_t)l.xo_p.size();
      l.xo_p.push_back(x.p);
      l.xo_slot.push_back(x.slot);
      l.keysum[q] += entry_hash(x.key, x.slot, max_rf);
    }
    l.xi_start[q] = (uint32_t)l.xi_p.size();
    for (const Entry& x : in[q]) {
      l.xi_p.push_back(x.p);
      l.xi_slot.push_back(x.slot);
      l.keysum_in[q] += entry_hash(x.key, x.slot, max_rf);
    }
  }
  l.xo_start[W] = (uint32_t)l.xo_p.size();
  l.xi_start[W] = (uint32_t)l.xi_p.size();
  for (uint32_t p = 0; p < P; ++p) {
    uint32_t k = 0;
    for (uint32_t s = 0; s < RF; ++s) k += l.outidx[(size_t)p * RF + s] != ~0u;
    l.max_remote = std::max(l.max_remote, k);
  }
  return l;
}

// The fixed-size words of the entries of peer q (two 8-byte words per entry: the acks and the commit
// notices), as a span of a [n][2] array whose entries are grouped by peer.
struct EntrySpan {
  uint64_t word = 0, bytes = 0;
};
inline EntrySpan entry_span(const std::vector<uint32_t>& start, uint32_t q) {
  return {2ull * start[q], 16ull * (start[q + 1] - start[q])};
}

// ---- buffer bounds

struct RegionConsts {
  uint64_t region_hdr = 0, dir_entry = 0, copy_chunk = 0;  // kRegionHdr, kDirEntry, kCopyChunk
};

struct BoundsShape {
  uint64_t group_max = 0, max_batch_records = 0, max_batch_bytes = 0, max_consumers = 0;
  uint32_t W = 0, RF = 0, max_remote = 0;
  uint64_t n_out = 0, n_in = 0;  // the lists' lengths
};

struct ReplBounds {
  uint64_t n_out = 0, n_in = 0;  // the per-entry arrays' lengths: the lists', at least 1
  uint64_t reserve = 0;          // catch-up bytes per destination (ro_catchup_reserve in the oracle)
  uint64_t dcap = 0;             // outbox bytes per destination
  uint64_t out_cap = 0, in_cap = 0, items_cap = 0;
};

// FORMAT.md §9 bounds: a record is at most 31 + L bytes in the log, sent once per remote slot, plus
// an 8-byte table slot; the catch-up reserve of a destination is one such round bound; per region a
// header, a directory, table padding and the consumer-offset rows.
inline ReplBounds plan_bounds(const BoundsShape& s, const RegionConsts& k) {
  ReplBounds b;
  b.n_in = std::max<uint64_t>(1, s.n_in);
  b.n_out = std::max<uint64_t>(1, s.n_out);
  const uint64_t rec = s.group_max * (39ull * s.max_batch_records + s.max_batch_bytes);
  const uint64_t per_entry = k.dir_entry + 16 + 8 * s.max_consumers;
  b.reserve = rec;
  b.dcap = ((uint64_t)s.max_remote * rec + b.reserve + k.region_hdr + 16 + per_entry * b.n_out + 255) & ~255ull;
  b.out_cap = (uint64_t)s.W * b.dcap;
  b.in_cap = (uint64_t)(s.W - 1) * ((uint64_t)(s.RF - 1) * rec + b.reserve + k.region_hdr + 32) + per_entry * b.n_in;
  b.items_cap = b.in_cap / k.copy_chunk + s.W + b.n_in;
  return b;
}

// ---- one round's layout

// From the landed sizes hs[4W] ([q]: {send bytes, send records}, then [W + q]: {recv bytes, recv
// records}): what goes to and comes from every peer, where the received regions lie in the inbox
// (packed in source order on 16 bytes), the verify tasks of each source and the copy work items.
struct RoundLayout {
  uint64_t sn[kPlanMaxWorld] = {}, rn[kPlanMaxWorld] = {};  // bytes sent to / received from q (0 for this rank)
  uint64_t soff[kPlanMaxWorld] = {};    // outbox offset of the region for q
  uint64_t region[kPlanMaxWorld] = {};  // inbox offset of the region from q (IngestArgs::region; ::rbytes is rn)
  uint32_t task0[kPlanMaxWorld + 1] = {};  // IngestArgs::task0
  uint64_t ro = 0;    // inbox bytes in use
  uint64_t smax = 0;  // the largest region sent
  uint32_t tasks = 0, items = 0;
};

// kvr: records per verify task; n_in: the in list's length. The caller refuses smax > dcap and ro > in_cap.
inline RoundLayout plan_round(const uint64_t* hs, uint32_t W, uint32_t me, uint64_t dcap, uint64_t kvr,
                              uint64_t items_cap, uint64_t n_in, uint64_t copy_chunk) {
  RoundLayout l;
  for (uint32_t q = 0; q < W; ++q) {
    l.sn[q] = q == me ? 0 : hs[2 * q];
    l.rn[q] = q == me ? 0 : hs[2 * W + 2 * q];
    l.soff[q] = (uint64_t)q * dcap;
    l.region[q] = l.ro;
    l.task0[q] = l.tasks;
    l.tasks += (uint32_t)((l.rn[q] ? hs[2 * W + 2 * q + 1] : 0) + kvr - 1) / kvr;
    l.smax = std::max(l.smax, l.sn[q]);
    l.ro += pad16(l.rn[q]);
  }
  l.task0[W] = l.tasks;
  // copy work items: at most one per copy chunk of received region bytes plus one per entry
  l.items = (uint32_t)std::min<uint64_t>(items_cap, l.ro / copy_chunk + W + n_in);
  return l;
}

}  // namespace rmq
