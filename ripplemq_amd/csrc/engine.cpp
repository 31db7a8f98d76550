// engine.cpp — host side of the C-ABI (include/ripplemq_engine.h): one engine (one HIP device) and
// all its device memory. This file keeps creation (the knobs from the environment, streams,
// allocations, initial state), destruction, the waits, caller memory, profiling and transport
// attach; engine_internal.hpp says which file holds the other calls.
#include <chrono>
#include <climits>

#include "engine_internal.hpp"

using namespace rmq;

namespace rmq {

uint32_t host_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int k = 31; k >= 0; --k) {
    if ((a >> k) & 1u) p ^= b;
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  }
  return p;
}

// Inverse of a in GF(2)[x] mod P (reflected), by Gaussian elimination of y -> y * a.
uint32_t host_inverse(uint32_t a) {
  uint32_t col[32];
  for (int k = 0; k < 32; ++k) col[k] = host_mulmod(1u << k, a);  // image of basis vector bit k
  // solve sum_k y_k col[k] = one (x^0 = 0x80000000): rows = output bits
  uint32_t rows[32];  // rows[b]: bit k = bit b of col[k]; bit 32 handled separately
  uint32_t rhs = 0;
  for (int bb = 0; bb < 32; ++bb) {
    rows[bb] = 0;
    for (int k = 0; k < 32; ++k) rows[bb] |= ((col[k] >> bb) & 1u) << k;
    rhs |= ((0x80000000u >> bb) & 1u) << bb;
  }
  int r = 0;
  int piv[32];
  for (int k = 0; k < 32 && r < 32; ++k) {
    int sel = -1;
    for (int bb = r; bb < 32; ++bb)
      if ((rows[bb] >> k) & 1u) { sel = bb; break; }
    if (sel < 0) continue;
    std::swap(rows[sel], rows[r]);
    const uint32_t t = (rhs >> sel) & 1u, u = (rhs >> r) & 1u;
    rhs = (rhs & ~((1u << sel) | (1u << r))) | (u << sel) | (t << r);
    for (int bb = 0; bb < 32; ++bb)
      if (bb != r && ((rows[bb] >> k) & 1u)) {
        rows[bb] ^= rows[r];
        rhs ^= ((rhs >> r) & 1u) << bb;
      }
    piv[r] = k;
    ++r;
  }
  uint32_t y = 0;
  for (int q = 0; q < r; ++q)
    if ((rhs >> q) & 1u) y |= 1u << piv[q];
  return y;
}

void build_crc_consts(CrcConsts* c) {
  for (uint32_t b = 0; b < 256; ++b) {
    uint32_t x = b;
    for (int k = 0; k < 8; ++k) x = (x >> 1) ^ (kCrcPoly & (0u - (x & 1u)));
    c->table[0][b] = x;
  }
  for (uint32_t t = 1; t < 8; ++t)
    for (uint32_t b = 0; b < 256; ++b)
      c->table[t][b] = (c->table[t - 1][b] >> 8) ^ c->table[0][c->table[t - 1][b] & 0xFF];
  uint32_t x2n[40];
  x2n[0] = 0x40000000u;  // x^1 in the reflected representation
  for (int k = 1; k < 40; ++k) x2n[k] = host_mulmod(x2n[k - 1], x2n[k - 1]);
  for (uint32_t k = 0; k < 2; ++k)  // shift past 16 << k zero bytes = multiply by x^(2^(7+k))
    for (uint32_t i = 0; i < 4; ++i)
      for (uint32_t b = 0; b < 256; ++b) c->zshift[k][i][b] = host_mulmod(b << (8 * i), x2n[7 + k]);
  for (uint32_t i = 0; i < 4; ++i)  // 1024 bytes = 2^13 bits
    for (uint32_t b = 0; b < 256; ++b) c->zshift1k[i][b] = host_mulmod(b << (8 * i), x2n[13]);
  uint32_t x128e = 0x80000000u;  // x^(128 e), e = 0..63
  for (uint32_t e = 0; e < 64; ++e) {
    c->sh16[e] = x128e;
    x128e = host_mulmod(x128e, x2n[7]);
  }
  uint32_t x8n = 0x80000000u;  // x^(8n), n = 0..15
  for (uint32_t n = 0; n < 16; ++n) {
    c->inv_pad[n] = n ? host_inverse(x8n) : 0x80000000u;
    c->inv_pad16[n] = host_mulmod(c->inv_pad[n], x2n[4]);
    x8n = host_mulmod(x8n, x2n[3]);
  }
  // nibble tables of the sixteen LDS tables of stage 3 (table[0..7], then zshift[0][0..3],
  // zshift[1][0..3], as laid out in LDS): each is GF(2)-linear in its byte
  for (uint32_t q = 0; q < 16; ++q) {
    const uint32_t* t = q < 8 ? c->table[q] : c->zshift[(q - 8) / 4][(q - 8) % 4];
    for (uint32_t n = 0; n < 16; ++n) {
      c->nib[q][n] = t[n];
      c->nib[q][16 + n] = t[n << 4];
    }
  }
}

bool is_pow2(uint64_t v) { return v && !(v & (v - 1)); }

uint32_t ilog2(uint64_t v) {
  uint32_t r = 0;
  while ((1ull << r) < v) ++r;
  return r;
}

// A fault of earlier work on the pipeline stream (kernels report nothing else: every rejection is
// a per-record status). Asynchronous errors are sticky, so a query sees them without a copy.
int check_err(rmq_engine* e) {
  const hipError_t q = hipStreamQuery(e->main_s);
  return q == hipSuccess || q == hipErrorNotReady ? RMQ_OK : hip_fail(q);
}

// Wait for everything issued on stream s. A blocking hipStreamSynchronize returns ~10 us after the
// last kernel ends (interrupt wake-up); a sync sits on the producer's path (rmq_sync, a poll that
// needs commit indices), so poll the stream for up to 20 ms first, then block.
// Wait for an event the same way: a blocking hipEventSynchronize now and then woke milliseconds
// late (8 ms stalls in one synchronous fetch of ten, round 4), so spin on queries first.
template <typename T>
static int spin_then_block(T what, hipError_t (*query)(T), hipError_t (*block)(T)) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t q = query(what);
    if (q == hipSuccess) return RMQ_OK;
    if (q != hipErrorNotReady) return hip_fail(q);
    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
  }
  HIP_TRY(block(what));
  return RMQ_OK;
}

int event_wait(hipEvent_t ev) { return spin_then_block(ev, hipEventQuery, hipEventSynchronize); }

int stream_wait(hipStream_t s) { return spin_then_block(s, hipStreamQuery, hipStreamSynchronize); }

hipEvent_t pool_event(rmq_engine* e) {
  if (!e->ev_pool.empty()) {
    hipEvent_t ev = e->ev_pool.back();
    e->ev_pool.pop_back();
    return ev;
  }
  hipEvent_t ev = nullptr;
  if (hipEventCreate(&ev) != hipSuccess) return nullptr;
  return ev;
}

// The pipeline advances the double-buffered log end only for partitions this engine leads; before
// a partition changes role, both state sets must hold its current log end (engine drained).
int equalize_state_sets(rmq_engine* e) {
  const StateSet other = e->sets[(e->applied + 1) & 1u];
  const size_t bytes = (size_t)e->cfg.num_partitions * 8;
  HIP_TRY(hipMemcpy(other.leo, e->st.leo, bytes, hipMemcpyDeviceToDevice));
  HIP_TRY(hipMemcpy(other.used, e->st.used, bytes, hipMemcpyDeviceToDevice));
  return RMQ_OK;
}

void free_engine(rmq_engine* e) {
  if (!e) return;
  hipSetDevice(e->device);
  if (e->main_s) {
    // every submitted batch is applied before the memory goes away; with a replication transport
    // a flush is collective, so the application must have called rmq_sync on every rank
    (void)fetch_flush(e);
    if (!e->repl) flush(e);
    hipStreamSynchronize(e->main_s);
    if (e->rank_s) hipStreamSynchronize(e->rank_s);
    dump_stamps(e);
  }
  // what a subsystem grows and replaces during the engine's life, by its subsystem
  repl_free(e);
  audit_free(e);
  repair_remote_free(e);
  fetch_free(e);
  lag_free(e);
  if (e->lag.ev) hipEventDestroy(e->lag.ev);
  unpack_free(e);
  staging_free(e);
  offsets_free(e);
  if (e->state_stage) hipHostFree(e->state_stage);
  // what lives as long as the engine, as recorded at its allocation
  for (void* p : e->owned_dev) hipFree(p);
  for (void* p : e->owned_host) hipHostFree(p);
  if (e->ev_main) hipEventDestroy(e->ev_main);
  for (hipEvent_t ev : e->ev_rank)
    if (ev) hipEventDestroy(ev);
  if (e->ev_pre_rank) hipEventDestroy(e->ev_pre_rank);
  if (e->rank_s) hipStreamDestroy(e->rank_s);
  if (e->fetch_out_s) hipStreamDestroy(e->fetch_out_s);
  if (e->copy_s) hipStreamDestroy(e->copy_s);
  for (auto& v : e->prof)
    for (EvPair& p : v) {
      if (p.a) hipEventDestroy(p.a);
      if (p.b) hipEventDestroy(p.b);
    }
  for (hipEvent_t ev : e->ev_pool) hipEventDestroy(ev);
  if (e->region.t0) hipEventDestroy(e->region.t0);
  if (e->region.t1) hipEventDestroy(e->region.t1);
  if (e->main_s) hipStreamDestroy(e->main_s);
  delete e;
}

int validate_cfg(const rmq_config* c) {
  if (!c) return RMQ_EINVAL;
  if (c->num_partitions == 0 || c->num_partitions > kMaxPartitions) return RMQ_EINVAL;
  if (c->replication_factor == 0 || c->replication_factor > RMQ_MAX_RF) return RMQ_EINVAL;
  if (!is_pow2(c->index_interval) || c->index_interval < 64 || c->index_interval > (1u << 20))
    return RMQ_EINVAL;
  if (!is_pow2(c->segment_bytes) || c->segment_bytes < 4ull * c->index_interval) return RMQ_EINVAL;
  if (c->max_consumers == 0) return RMQ_EINVAL;
  if (c->max_batch_records == 0 || c->max_batch_records > kMaxBatchRecords) return RMQ_EINVAL;
  if (c->max_batch_bytes >= (1ull << 32)) return RMQ_EINVAL;
  if (c->pipeline_depth > kMaxGroup) return RMQ_EINVAL;
  const uint64_t g = c->pipeline_depth ? c->pipeline_depth : 2u;
  const uint64_t pool = c->pool_bytes ? c->pool_bytes : (uint64_t)c->num_partitions * c->segment_bytes;
  if (pool < (uint64_t)c->num_partitions * c->segment_bytes || pool % c->index_interval) return RMQ_EINVAL;
  if ((2 * g + 2) * (pool / c->index_interval) >= (1ull << 40)) return RMQ_EINVAL;
  return RMQ_OK;
}

namespace {

// The environment, read once by rmq_create: {variable, the knob it sets, the least value it takes}.
const struct {
  const char* env;
  uint32_t Knobs::*field;
  int min = INT_MIN;
} kKnobs[] = {
    {"RMQ_TRACE", &Knobs::trace},           {"RMQ_DEBUG", &Knobs::debug},
    {"RMQ_WG3_ALL", &Knobs::wg3_all},       {"RMQ_S1_WGS", &Knobs::s1_wgs},
    {"RMQ_S2_WGS", &Knobs::s2_wgs},         {"RMQ_S3_FIRST", &Knobs::s3_first},
    {"RMQ_PRIO", &Knobs::prio},             {"RMQ_S3_LEAD", &Knobs::s3_lead},
    {"RMQ_RANK", &Knobs::rank_mode},        {"RMQ_STEAL", &Knobs::steal},
    {"RMQ_AHEAD", &Knobs::max_ahead},       {"RMQ_SPLIT", &Knobs::split},
    {"RMQ_S3_PAIR", &Knobs::s3_pair},       {"RMQ_S3_ROLES", &Knobs::s3_roles},
    {"RMQ_S3_STAGE", &Knobs::s3_stage},     {"RMQ_FETCH_COALESCE", &Knobs::fetch_coalesce},
    {"RMQ_S3_XCD", &Knobs::s3_xcd},         {"RMQ_S1_XCD", &Knobs::s1_xcd},
    {"RMQ_RANK_CUS", &Knobs::rank_cus},     {"RMQ_FETCH_DMA", &Knobs::fetch_dma},
    {"RMQ_FETCH_DMA_IN", &Knobs::fetch_dma_in}, {"RMQ_BIG_WGS", &Knobs::big_wgs},
    {"RMQ_VERIFY_WGS", &Knobs::verify_wgs, 1},  {"RMQ_AUDIT_WGS", &Knobs::audit_wgs, 0},
};
const struct {
  const char* env;
  uint64_t Knobs::*field;
} kKnobs64[] = {{"RMQ_STAMPS_AT", &Knobs::stamps_at}, {"RMQ_REPAIR_PEER_BYTES", &Knobs::repair_peer_bytes}};

void read_knobs(rmq_engine* e) {
  Knobs& k = e->knob;
  for (const auto& r : kKnobs)
    if (const char* v = std::getenv(r.env)) k.*r.field = (uint32_t)std::max(r.min, std::atoi(v));
  for (const auto& r : kKnobs64)
    if (const char* v = std::getenv(r.env)) k.*r.field = std::strtoull(v, nullptr, 10);
  e->stamps_path = std::getenv("RMQ_STAMPS");
  if (e->stamps_path || k.steal) k.split = 0;  // (phase stamps and stealing read one launch's roles)
}

#define TRY(x) do { if (int _r = (x)) return _r; } while (0)

int create_streams(rmq_engine* e) {
  const Knobs& k = e->knob;
  if (k.split && k.rank_cus && k.rank_cus < e->cu_count) {
    // CU masks (bit i = the i-th CU in the runtime's numbering): the rank stream takes the first
    // rank_cus bits, the pipeline stream the rest
    std::vector<uint32_t> mr((e->cu_count + 31) / 32, 0u), mm(mr.size(), 0u);
    for (uint32_t i = 0; i < e->cu_count; ++i) (i < k.rank_cus ? mr : mm)[i / 32] |= 1u << (i % 32);
    HIP_TRY(hipExtStreamCreateWithCUMask(&e->main_s, (uint32_t)mm.size(), mm.data()));
    HIP_TRY(hipExtStreamCreateWithCUMask(&e->rank_s, (uint32_t)mr.size(), mr.data()));
  } else {
    HIP_TRY(hipStreamCreateWithFlags(&e->main_s, hipStreamNonBlocking));
    if (k.split) HIP_TRY(hipStreamCreateWithFlags(&e->rank_s, hipStreamNonBlocking));
  }
  if (k.split) {
    for (hipEvent_t& ev : e->ev_rank) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->ev_pre_rank, hipEventDisableTiming));
  }
  HIP_TRY(hipStreamCreateWithFlags(&e->fetch_out_s, hipStreamNonBlocking));
  preload_fetch_kernels();
  HIP_TRY(hipStreamCreateWithFlags(&e->copy_s, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&e->ev_main, hipEventDisableTiming));
  for (rmq_engine::FetchSlot& f : e->fslot) {
    HIP_TRY(hipEventCreateWithFlags(&f.ev, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&f.ev_copy, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&f.ev_in, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&f.ev_k, hipEventDisableTiming));
  }
  return RMQ_OK;
}

// The partitions' state, logs, index and consumer tables (dalloc zero-fills: every log empty, every
// replica cursor at offset 0), and every partition's first ring.
int alloc_state(rmq_engine* e) {
  const rmq_config& cfg = e->cfg;
  const uint32_t P = cfg.num_partitions, RF = cfg.replication_factor, C = cfg.max_consumers;
  DevState& s = e->st;
  s.P = P;
  s.RF = RF;
  s.C = C;
  s.interval_log2 = ilog2(cfg.index_interval);
  e->group_max = std::min<uint32_t>(kMaxGroup, cfg.pipeline_depth);
  // stage 4 reads a group's index entries while stage 3 of the group two later writes new ones
  // (each batch adds at most ring - interval bytes to a partition): 2G + 1 rings' worth of entries
  // (+2) keep every entry stage 4 may read from being overwritten in time; (2G + 2) per interval
  // of ring covers that for every ring of at least 4 intervals
  s.icap_mul = 2u * e->group_max + 2u;
  s.rstride = cfg.pool_bytes ? cfg.pool_bytes : (uint64_t)P * cfg.segment_bytes;
  e->pool.size = s.rstride;
  e->ring.assign(P, 0);
  for (uint32_t p = 0; p < P; ++p) {  // every partition starts with a segment_bytes ring
    uint64_t off = 0;
    const uint32_t lg = ilog2(cfg.segment_bytes);
    if (!e->pool.alloc(lg, &off)) return RMQ_EINVAL;
    e->ring[p] = off | lg;
  }
  for (StateSet& z : e->sets) {
    TRY(owned_dalloc(e, &z.leo, P));
    TRY(owned_dalloc(e, &z.used, P));
  }
  s.leo = e->sets[0].leo;
  s.used = e->sets[0].used;
  // (in this order: the order of the allocations decides where the arrays lie on the device)
  TRY(owned_dalloc(e, &s.start_off, P));
  TRY(owned_dalloc(e, &s.start_pos, P));
  TRY(owned_dalloc(e, &s.commit, P));
  TRY(owned_dalloc(e, &s.hw, P));
  TRY(owned_dalloc(e, &s.term_start, P));
  TRY(owned_dalloc(e, &s.term, P));
  TRY(owned_dalloc(e, &s.match, (size_t)P * RF));
  TRY(owned_dalloc(e, &s.is_leader, P));
  TRY(owned_dalloc(e, &s.local_mask, P));
  TRY(owned_dalloc(e, &s.index, (size_t)(s.rstride >> s.interval_log2) * s.icap_mul * 2));
  TRY(owned_dalloc(e, &s.logs, (size_t)RF * s.rstride));
  TRY(owned_dalloc(e, &s.ring, P));
  TRY(owned_dalloc(e, &s.cons, (size_t)P * C));
  TRY(owned_dalloc(e, &s.pcache, (size_t)P * C * 2));
  TRY(owned_dalloc(e, &s.rcur, P));
  uint64_t** const later[] = {&s.lcommit, &s.lterm, &s.mterm, &s.heard, &s.cver, &s.cq};
  TRY(owned_dalloc(e, &s.cdirty, P));
  for (uint64_t** p : later) TRY(owned_dalloc(e, p, P));
  TRY(owned_dalloc(e, &e->d_rlate, P));
  HIP_TRY(hipMemcpy(s.ring, e->ring.data(), (size_t)P * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(s.pcache, 0xFF, (size_t)P * C * 16));  // every entry empty
  e->cver.assign(P, 0ull);
  return RMQ_OK;
}

// The ticket stats ring, the pipeline's scratch sets and the stamps of RMQ_STAMPS.
int alloc_scratch(rmq_engine* e) {
  const uint32_t P = e->cfg.num_partitions;
  e->max_tiles = (e->cfg.max_batch_records + kTileRecs - 1) / kTileRecs;
  e->max_tasks = (e->cfg.max_batch_records + kTaskRecs - 1) / kTaskRecs;
  TRY(owned_dalloc(e, &e->d_stats, (size_t)kStatsRing * e->max_tasks));
  // a multiple of four: stage 2 reads u32 hist columns with 16-byte loads
  e->max_group_tiles = (std::min<uint32_t>(kMaxTiles, e->group_max * e->max_tiles) + 3u) & ~3u;
  for (PipeScratch& x : e->scratch) {
    const size_t GT = e->max_group_tiles, TP = GT * P;
    TRY(owned_dalloc(e, &x.hist32, TP));
    TRY(owned_dalloc(e, &x.hist, TP));
    TRY(owned_dalloc(e, &x.excl, TP));
    TRY(owned_dalloc(e, &x.totals, P));
    TRY(owned_dalloc(e, &x.pk, (size_t)P * 8));
    TRY(owned_dalloc(e, &x.bcum, (size_t)kMaxGroup * P));
    TRY(owned_dalloc(e, &x.crank, GT * kTileRecs));
    TRY(owned_dalloc(e, &x.pre, GT * kTileRecs));
    TRY(owned_dalloc(e, &x.tsum, GT * 4));
    TRY(owned_dalloc(e, &x.tile_base, GT));
    TRY(owned_dalloc(e, &x.binfo, (size_t)kMaxGroup * 4));
    TRY(owned_dalloc(e, &x.bacc, (size_t)kMaxGroup * 2));
    TRY(owned_dalloc(e, &x.nbig, 4));
    TRY(owned_dalloc(e, &x.bigl, GT * kTileRecs));
  }
  if (e->stamps_path)
    TRY(owned_dalloc(e, &e->d_stamps, (size_t)(2u * e->cu_count + kMaxTiles + (P + kPipeThreads - 1) / kPipeThreads +
                                               kMaxTiles * kTileRecs / (kTaskRecs * kPipeThreads / 64)) * 64));
  return RMQ_OK;
}

// The coherent page-locked words kernels report through: each fetch slot's bytes and table words
// needed, and the pipeline's done words.
int alloc_host_words(rmq_engine* e) {
  const unsigned flags = hipHostMallocCoherent | hipHostMallocMapped;
  TRY(owned_host_alloc(e, &e->fetch_need_host, 16 * rmq_engine::kFetchSlots, flags));
  for (uint32_t k = 0; k < rmq_engine::kFetchSlots; ++k) {
    rmq_engine::FetchSlot& f = e->fslot[k];
    f.need = e->fetch_need_host + k;
    f.tneed = e->fetch_need_host + rmq_engine::kFetchSlots + k;
    *f.need = *f.tneed = 0;
    HIP_TRY(hipHostGetDevicePointer((void**)&f.need_dev, f.need, 0));
    HIP_TRY(hipHostGetDevicePointer((void**)&f.tneed_dev, f.tneed, 0));
  }
  TRY(owned_host_alloc(e, &e->done_host, 64, flags));
  e->done_host[0] = e->done_host[1] = 0;
  HIP_TRY(hipHostGetDevicePointer((void**)&e->done_dev, e->done_host, 0));
  return RMQ_OK;
}

// The CRC constants, and every partition led here from term 1 with all its replicas local.
int init_state(rmq_engine* e) {
  const uint32_t P = e->cfg.num_partitions, RF = e->cfg.replication_factor, rank = e->cfg.rank;
  DevState& s = e->st;
  {
    CrcConsts h;
    build_crc_consts(&h);
    TRY(owned_dalloc(e, &e->d_crc, 1));
    HIP_TRY(hipMemcpy(e->d_crc, &h, sizeof h, hipMemcpyHostToDevice));
  }
  e->is_leader.assign(P, 1u);
  TRY(write_words(s.is_leader, e->is_leader));
  TRY(write_words(s.local_mask, std::vector<uint32_t>(P, (1u << RF) - 1u)));
  e->leader_slot.assign(P, 0u);
  e->ranks.assign((size_t)P * RF, rank);
  e->term.assign(P, 1ull);
  TRY(write_words(s.term, e->term));
  // every partition is led here from term 1 (its leader-start entry, its own vote)
  TRY(write_words(s.lterm, e->term));
  TRY(write_words(s.mterm, e->term));
  e->vterm.assign(P, 1ull);
  e->vfor.assign(P, rank);
  e->vled.assign(P, 1u);
  e->key.resize(P);
  for (uint32_t p = 0; p < P; ++p) e->key[p] = p;
  e->ticket_n.assign(kStatsRing, 0u);
  uint32_t bits = 0;
  while ((1u << bits) < P) ++bits;  // keys in [0, P)
  e->key_passes = bits == 0 ? 0u : bits <= 8 ? 1u : 2u;
  e->key_bits = bits;
  e->staging.resize(4u * e->group_max + 1u);  // batches of the forming group and of three in flight
  return RMQ_OK;
}

int create_engine(rmq_engine* e) {
  read_knobs(e);
  HIP_TRY(hipSetDevice(e->device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, e->device));
  e->cu_count = (uint32_t)prop.multiProcessorCount;
  if (!e->knob.verify_wgs) e->knob.verify_wgs = verify_wgs_per_cu() * e->cu_count;
  std::snprintf(e->dev_name, sizeof e->dev_name, "%s (%s)", prop.name, prop.gcnArchName);
  TRY(create_streams(e));
  TRY(alloc_state(e));
  TRY(alloc_scratch(e));
  TRY(alloc_host_words(e));
  TRY(init_state(e));
  HIP_TRY(hipDeviceSynchronize());
  return RMQ_OK;
}
#undef TRY

}  // namespace

}  // namespace rmq

extern "C" {

uint32_t rmq_abi_version(void) { return RMQ_ABI_VERSION; }

int rmq_host_alloc(rmq_engine* e, uint64_t bytes, void** out) {
  if (!e || !out || !bytes) return RMQ_EINVAL;
  HIP_TRY(hipSetDevice(e->device));
  *out = nullptr;
  if (hipHostMalloc(out, bytes, 0) != hipSuccess) return RMQ_ENOMEM;
  return RMQ_OK;
}

int rmq_host_free(rmq_engine* e, void* p) {  // e may be NULL (after rmq_destroy)
  (void)e;
  if (p && hipHostFree(p) != hipSuccess) return RMQ_EDEVICE;
  return RMQ_OK;
}

int rmq_host_register(rmq_engine* e, void* p, uint64_t bytes) {
  if (!e || !p || !bytes) return RMQ_EINVAL;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
  return RMQ_OK;
}

int rmq_host_unregister(rmq_engine* e, void* p) {
  if (!e || !p) return RMQ_EINVAL;
  HIP_TRY(hipHostUnregister(p));
  return RMQ_OK;
}

const char* rmq_strerror(int s) {
  switch (s) {
    case RMQ_OK: return "ok";
    case RMQ_PENDING: return "pending";
    case RMQ_ENOTLEADER: return "Not leader";
    case RMQ_ENOPART: return "unknown partition";
    case RMQ_EINVAL: return "invalid argument";
    case RMQ_ENOSPC: return "no space";
    case RMQ_EDEVICE: return "device error";
    case RMQ_EOFFSET: return "offset out of range";
    case RMQ_ENOMEM: return "out of memory";
    case RMQ_ESTALE: return "replica lags the committed log";
    case RMQ_ETERM: return "term already led or voted for another candidate";
    case RMQ_ECORRUPT: return "record checksum or log structure is corrupt";
    default: return "unknown status";
  }
}

void rmq_config_default(rmq_config* c, uint32_t P, uint32_t RF) {
  if (!c) return;
  std::memset(c, 0, sizeof *c);
  c->num_partitions = P;
  c->replication_factor = RF;
  c->segment_bytes = 1ull << 20;
  c->index_interval = 1024;
  c->max_consumers = 8;
  c->max_batch_records = 65536;
  c->pipeline_depth = 2;
  c->max_batch_bytes = 64ull << 20;
  c->device = 0;
  c->rank = 0;
}

int rmq_create(const rmq_config* cfg, rmq_engine** out) {
  if (!out) return RMQ_EINVAL;
  *out = nullptr;
  int rc = validate_cfg(cfg);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev)
    return RMQ_EDEVICE;
  rmq_engine* e = new (std::nothrow) rmq_engine();
  if (!e) return RMQ_ENOMEM;
  e->cfg = *cfg;
  if (!e->cfg.pipeline_depth) e->cfg.pipeline_depth = 2;
  e->device = cfg->device;
  rc = create_engine(e);
  if (rc) {
    free_engine(e);  // (works on a half-built engine: whatever was recorded or set so far)
    return rc;
  }
  *out = e;
  return RMQ_OK;
}

void rmq_destroy(rmq_engine* e) { free_engine(e); }

int rmq_device_alloc(rmq_engine* e, uint64_t bytes, void** out) {
  if (!e || !out) return RMQ_EINVAL;
  EngineLock g(e);
  HIP_TRY(hipSetDevice(e->device));
  *out = nullptr;
  HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
  return RMQ_OK;
}

int rmq_device_free(rmq_engine* e, void* p) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  int rc = begin_call(e, settle);
  if (rc) return rc;
  if (p) HIP_TRY(hipFree(p));
  return RMQ_OK;
}

int rmq_memcpy(rmq_engine* e, void* dst, const void* src, uint64_t bytes, int kind) {
  if (!e || (bytes && (!dst || !src))) return RMQ_EINVAL;
  EngineLock g(e);
  HIP_TRY(hipSetDevice(e->device));
  const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice
                        : kind == 1 ? hipMemcpyDeviceToHost
                                    : hipMemcpyDeviceToDevice;
  int rc = settle(e);
  if (rc) return rc;
  if (bytes) HIP_TRY(hipMemcpy(dst, src, bytes, k));
  return RMQ_OK;
}

int rmq_profile_enable(rmq_engine* e, int enable) {
  if (!e) return RMQ_EINVAL;
  EngineLock g(e);
  int rc = begin_call(e, settle);
  if (rc) return rc;
  for (auto& v : e->prof) {
    for (EvPair& p : v) {
      e->ev_pool.push_back(p.a);
      e->ev_pool.push_back(p.b);
    }
    v.clear();
  }
  e->profile = enable > 0 ? 1u : 0u;
  e->fetch_replay = enable > 1 ? (uint32_t)enable : 1u;
  e->region.launches = e->region.batches = e->prof_fetch_runs = 0;
  e->region.started = e->region.ended = false;
  if (e->profile && !e->region.t0) {
    HIP_TRY(hipEventCreate(&e->region.t0));
    HIP_TRY(hipEventCreate(&e->region.t1));
  }
  return RMQ_OK;
}

int rmq_profile_query(rmq_engine* e, int kernel, uint64_t* launches, double* total_ms) {
  if (!e || kernel < 0 || kernel > 11) return RMQ_EINVAL;
  EngineLock g(e);
  int rc = begin_call(e, settle);
  if (rc) return rc;
  if (kernel <= 1) {  // 0: pipeline launches in the region, 1: batches applied in it
    float ms = 0;
    if (e->region.ended) HIP_TRY(hipEventElapsedTime(&ms, e->region.t0, e->region.t1));
    if (launches) *launches = e->region.ended ? (kernel ? e->region.batches : e->region.launches) : 0;
    if (total_ms) *total_ms = ms;
    return RMQ_OK;
  }
  double tot = 0;
  for (const EvPair& p : e->prof[kernel]) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, p.a, p.b));
    tot += ms;
  }
  if (launches) *launches = kernel == 4 ? e->prof_fetch_runs : e->prof[kernel].size();
  if (total_ms) *total_ms = tot;
  return RMQ_OK;
}

int rmq_device_info(rmq_engine* e, char* name, uint32_t name_cap, uint32_t* cu_count) {
  if (!e) return RMQ_EINVAL;
  if (name && name_cap) std::snprintf(name, name_cap, "%s", e->dev_name);
  if (cu_count) *cu_count = e->cu_count;
  return RMQ_OK;
}

int rmq_rccl_unique_id(uint8_t* out) {
  if (!out) return RMQ_EINVAL;
  return rccl_unique_id(out);
}

int rmq_attach_rccl(rmq_engine* e, const uint8_t* comm_id, uint32_t world) {
  if (!e || !comm_id || world < 2 || world > kMaxWorld) return RMQ_EINVAL;
  EngineLock g(e);
  if (e->repl) return RMQ_EINVAL;
  int rc = begin_call(e, drain);
  if (rc) return rc;
  Transport* t = make_rccl_transport(comm_id, world, e->cfg.rank);
  if (!t) return RMQ_EDEVICE;
  rc = repl_attach(e, t);
  if (rc && !e->repl) delete t;
  return rc;
}

struct rmq_local_hub {
  rmq::LocalHub hub;
  explicit rmq_local_hub(uint32_t w) : hub(w) {}
};

int rmq_local_hub_create(uint32_t world, rmq_local_hub** out) {
  if (!out || world < 2 || world > kMaxWorld) return RMQ_EINVAL;
  *out = new (std::nothrow) rmq_local_hub(world);
  return *out ? RMQ_OK : RMQ_ENOMEM;
}

void rmq_local_hub_destroy(rmq_local_hub* h) { delete h; }

int rmq_attach_local(rmq_engine* e, rmq_local_hub* h) {
  if (!e || !h) return RMQ_EINVAL;
  EngineLock g(e);
  if (e->repl) return RMQ_EINVAL;
  int rc = begin_call(e, drain);
  if (rc) return rc;
  Transport* t = make_local_transport(&h->hub, e->cfg.rank, e->device);
  rc = repl_attach(e, t);
  if (rc && !e->repl) delete t;
  return rc;
}

}  // extern "C"
