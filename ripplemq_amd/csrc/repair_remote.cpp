// repair_remote.cpp — the collective rounds of rmq_repair_remote (FORMAT.md §10 "Remote repair").
//
// After rmq_repair's first pass (audit.cpp) every rank plays RF - 1 rounds, the same sequence of
// Transport::exchange calls on each: round j asks candidate j of every partition for the pairs still
// failing. A round is {request bytes, pairs that want a candidate} words all-to-all (every rank sees
// every count: all stop together once all are zero), the request lists, the serve kernels on the
// donor, the response sizes, the responses, the install kernel on the requester (repair_remote.hip).
// The request and install kernels run on the pipeline stream, the exchanges and the serve kernels on
// the exchange stream, ordered by an event as post_round orders them; the host waits wherever a
// size must be known on the host (the transport takes host-side byte counts), which is several times
// a round: the call is a rare control-plane call and its cost is unmeasured.
//
// Sizes that arrive over the transport are checked against what this rank can derive itself before a
// buffer is sized from them: a request list is at most kRemoteMaxReqs requests, a response at most
// header + directory + the segment bytes this rank asked of that peer.
#include "engine_internal.hpp"

namespace rmq {

namespace {

// The call's device buffers: dalloc and grow, the buffer noted on the record repair_remote_free frees from.
template <typename T>
int rr_alloc(rmq_engine::RemoteRepair& B, T** p, size_t count) {
  const int rc = dalloc(p, count);
  if (*p) B.dev.note(p);
  return rc;
}
template <typename T>
int rr_grow(rmq_engine::RemoteRepair& B, T** p, uint64_t* cap, uint64_t need) {
  if (!*p) B.dev.note(p);  // (grow keeps the pointer's address)
  return grow(p, cap, need);
}

int swap_words(rmq_engine* e, uint32_t W) {
  rmq_engine::RemoteRepair& B = e->rr;
  Replication* r = e->repl;
  HIP_TRY(hipMemcpyAsync(B.words + kRemoteWSend, B.h_words + kRemoteWSend, 2ull * W * 8, hipMemcpyHostToDevice, r->xchg_s));
  int rc = fixed_swap(r, B.words + kRemoteWSend, B.words + kRemoteWRecv, 2, 16).post(r);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(B.h_words + kRemoteWRecv, B.words + kRemoteWRecv, 2ull * W * 8, hipMemcpyDeviceToHost, r->xchg_s));
  HIP_TRY(hipStreamSynchronize(r->xchg_s));
  return RMQ_OK;
}

}  // namespace

void repair_remote_free(rmq_engine* e) {
  rmq_engine::RemoteRepair& B = e->rr;
  B.dev.free_all();
  if (B.h_words) hipHostFree(B.h_words);
  if (B.ev) hipEventDestroy(B.ev);
  B = rmq_engine::RemoteRepair();
}

int repair_remote_rounds(rmq_engine* e, const RepairArgs* a, uint32_t wgs, uint64_t tasks, uint64_t* fetched,
                         uint64_t* served) {
  Replication* r = e->repl;
  rmq_engine::RemoteRepair& B = e->rr;
  const uint32_t W = r->world, me = r->rank, RF = e->cfg.replication_factor, P = e->cfg.num_partitions;
  const uint32_t ncand = RF - 1u;
  const bool dry = a && !a->write;
  served[0] = served[1] = 0;
  int rc = RMQ_OK;
  if (!B.words) {
    rc = rr_alloc(B, &B.words, kRemoteWords);
    if (!rc) rc = rr_alloc(B, &B.csum, (size_t)kMaxWorld * kRemoteChunks);
    if (rc) return rc;
    HIP_TRY(hipHostMalloc((void**)&B.h_words, (kRemoteWords + 2ull * kMaxWorld) * 8, 0));
    HIP_TRY(hipEventCreateWithFlags(&B.ev, hipEventDisableTiming));
  }
  uint64_t* hw = B.h_words;
  uint64_t* hh = hw + kRemoteWords;  // the list headers of a round, 16 bytes per destination
  // what a donor resolves a request's key with: {key, pidx} ascending by key
  {
    std::vector<RemoteKey> keys(P);
    for (uint32_t p = 0; p < P; ++p) keys[p] = {e->key[p], p, 0u};
    std::sort(keys.begin(), keys.end(), [](const RemoteKey& x, const RemoteKey& y) { return x.key < y.key; });
    uint64_t cap = B.key_cap;
    rc = rr_grow(B, &B.keys, &cap, P);
    if (!rc) rc = rr_grow(B, &B.pkey, &B.key_cap, P);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(B.keys, keys.data(), (size_t)P * sizeof(RemoteKey), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(B.pkey, e->key.data(), (size_t)P * 8, hipMemcpyHostToDevice));
  }
  uint32_t max_reqs = 0, n = 0;
  uint64_t list_cap = 0;
  if (a && ncand) {
    n = a->s.n;
    // donor candidates: the leader's rank first, then the other slots' ranks ascending by slot,
    // without this rank and without duplicates
    std::vector<uint32_t> cand((size_t)n * ncand, ~0u);
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t p = a->s.first + i;
      const uint32_t* rk = &e->ranks[(size_t)p * RF];
      uint32_t* c = &cand[(size_t)i * ncand];
      uint32_t k = 0;
      auto add = [&](uint32_t q) {
        if (q == me || q >= W || k >= ncand || std::find(c, c + k, q) != c + k) return;
        c[k++] = q;
      };
      add(rk[e->leader_slot[p]]);
      for (uint32_t s = 0; s < RF; ++s) add(rk[s]);
    }
    max_reqs = (uint32_t)std::min<uint64_t>(kRemoteMaxReqs, std::max<uint64_t>(tasks, 1));
    list_cap = kRemoteHdr + (uint64_t)kRemoteReq * max_reqs;
    rc = rr_grow(B, &B.cand, &B.cand_cap, cand.size());
    if (!rc) rc = rr_grow(B, &B.want, &B.want_cap, tasks);
    if (!rc) rc = rr_grow(B, &B.fetched, &B.fetched_cap, 2ull * n);
    if (!rc) rc = rr_grow(B, &B.lists, &B.lists_cap, (uint64_t)W * list_cap);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(B.cand, cand.data(), cand.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(B.fetched, 0, 2ull * n * 8, e->main_s));
  }
  Exchange x;  // the request lists, then the responses
  for (uint32_t j = 0; j < ncand; ++j) {
    uint32_t nreq[kMaxWorld] = {};
    uint64_t asked[kMaxWorld] = {};
    uint64_t remain = 0;
    if (n) {
      HIP_TRY(hipMemsetAsync(B.words + kRemoteWCtr, 0, (2ull * W + 1) * 8, e->main_s));
      RemoteReqArgs q{};
      q.r = *a;
      q.want = B.want;
      q.cand = B.cand;
      q.pkey = B.pkey;
      q.lists = B.lists;
      q.list_cap = list_cap;
      q.ctr = B.words + kRemoteWCtr;
      q.peer_bytes = e->knob.repair_peer_bytes;
      q.round = j;
      q.world = W;
      q.ncand = ncand;
      q.max_reqs = max_reqs;
      launch_remote_request(q, wgs, e->main_s);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(hw + kRemoteWCtr, B.words + kRemoteWCtr, (2ull * W + 1) * 8, hipMemcpyDeviceToHost, e->main_s));
      HIP_TRY(hipStreamSynchronize(e->main_s));
      for (uint32_t q2 = 0; q2 < W; ++q2) {
        nreq[q2] = q2 == me ? 0u : (uint32_t)std::min<uint64_t>(hw[kRemoteWCtr + q2], max_reqs);
        asked[q2] = hw[kRemoteWCtr + W + q2];
      }
      remain = hw[kRemoteWCtr + 2 * W];
    }
    // 1. {request bytes, pairs that want a candidate this round}, all-to-all
    for (uint32_t q = 0; q < W; ++q) {
      hw[kRemoteWSend + 2 * q] = nreq[q] ? kRemoteHdr + (uint64_t)kRemoteReq * nreq[q] : 0;
      hw[kRemoteWSend + 2 * q + 1] = remain;
      hh[2 * q] = (uint64_t)kRemoteMagic | ((uint64_t)nreq[q] << 32);
      hh[2 * q + 1] = (uint64_t)j | ((uint64_t)(dry ? kRemoteDry : 0u) << 32);
      if (nreq[q]) HIP_TRY(hipMemcpyAsync(B.lists + (uint64_t)q * list_cap, hh + 2 * q, 16, hipMemcpyHostToDevice, e->main_s));
    }
    HIP_TRY(hipEventRecord(B.ev, e->main_s));
    HIP_TRY(hipStreamWaitEvent(r->xchg_s, B.ev, 0));
    rc = swap_words(e, W);
    if (rc) return rc;
    bool any = remain != 0;
    for (uint32_t q = 0; q < W; ++q) any = any || (q != me && hw[kRemoteWRecv + 2 * q + 1] != 0);
    if (!any) break;  // (every rank read the same counts)
    // 2. the requests
    RemoteServeArgs S{};
    uint64_t ro = 0;
    uint32_t nin = 0;
    for (uint32_t q = 0; q < W; ++q) {
      const uint64_t nb = q == me ? 0 : hw[kRemoteWRecv + 2 * q];
      if (nb > kRemoteHdr + (uint64_t)kRemoteReq * kRemoteMaxReqs) {
        std::fprintf(stderr, "ripplemq: rank %u announced a repair request list of %llu bytes\n", q, (unsigned long long)nb);
        return RMQ_EDEVICE;
      }
      // (a list that is not a header and whole requests is answered with nothing)
      const uint32_t nq = nb > kRemoteHdr && (nb - kRemoteHdr) % kRemoteReq == 0 ? (uint32_t)((nb - kRemoteHdr) / kRemoteReq) : 0u;
      x.peer(q, B.lists + (uint64_t)q * list_cap, hw[kRemoteWSend + 2 * q], nullptr, nb);
      S.in_off[q] = ro;
      S.w0[q] = nin;
      ro += pad16(nb);
      nin += nq;
    }
    for (uint32_t q = W; q <= kMaxWorld; ++q) S.w0[q] = nin;
    rc = rr_grow(B, &B.rin, &B.rin_cap, std::max<uint64_t>(ro, 16));
    if (!rc) rc = rr_grow(B, &B.sv, &B.sv_cap, std::max<uint32_t>(nin, 1));
    if (rc) return rc;
    for (uint32_t q = 0; q < W; ++q) x.rb[q] = B.rin + S.in_off[q];
    rc = x.post(r);
    if (rc) return rc;
    // 3. the serve: verdicts and span bytes, then (the response sized from them) directory and spans
    S.st = e->st;
    S.crc = e->d_crc;
    S.keys = B.keys;
    S.nkeys = P;
    S.world = W;
    S.in = B.rin;
    S.sv = B.sv;
    S.csum = B.csum;
    S.tot = B.words + kRemoteWTot;
    HIP_TRY(hipMemsetAsync(B.csum, 0, (size_t)W * kRemoteChunks * 8, r->xchg_s));
    HIP_TRY(hipMemsetAsync(B.words + kRemoteWTot, 0, 3ull * W * 8, r->xchg_s));
    launch_remote_serve_check(S, r->xchg_s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hw + kRemoteWTot, B.words + kRemoteWTot, 3ull * W * 8, hipMemcpyDeviceToHost, r->xchg_s));
    HIP_TRY(hipStreamSynchronize(r->xchg_s));
    uint64_t oo = 0, resp[kMaxWorld] = {};
    for (uint32_t q = 0; q < W; ++q) {
      const uint32_t nq = S.w0[q + 1] - S.w0[q];
      resp[q] = nq ? kRemoteHdr + (uint64_t)kRemoteDir * nq + hw[kRemoteWTot + 3 * q + 2] : 0;
      S.out_off[q] = oo;
      oo += pad16(resp[q]);
      served[0] += hw[kRemoteWTot + 3 * q];
      served[1] += hw[kRemoteWTot + 3 * q + 1];
    }
    rc = rr_grow(B, &B.out, &B.out_cap, std::max<uint64_t>(oo, 16));
    if (rc) return rc;
    S.out = B.out;
    launch_remote_serve_copy(S, r->xchg_s);
    HIP_TRY(hipGetLastError());
    for (uint32_t q = 0; q < W; ++q) {  // rmq_fault_corrupt_repair
      if (!B.flip[q] || !resp[q]) continue;
      B.flip[q] = false;
      const int64_t data = (int64_t)hw[kRemoteWTot + 3 * q + 2];
      const int64_t at = B.flip_at[q] < 0 ? data + B.flip_at[q] : B.flip_at[q];
      if (at < 0 || at >= data) continue;
      uint8_t* byte = B.out + S.out_off[q] + (resp[q] - (uint64_t)data) + (uint64_t)at;
      uint8_t b = 0;
      HIP_TRY(hipStreamSynchronize(r->xchg_s));
      HIP_TRY(hipMemcpy(&b, byte, 1, hipMemcpyDeviceToHost));
      b ^= 0x5A;
      HIP_TRY(hipMemcpy(byte, &b, 1, hipMemcpyHostToDevice));
    }
    // 4. the response sizes
    for (uint32_t q = 0; q < W; ++q) {
      hw[kRemoteWSend + 2 * q] = resp[q];
      hw[kRemoteWSend + 2 * q + 1] = 0;
    }
    rc = swap_words(e, W);
    if (rc) return rc;
    // 5. the responses
    RemoteInstallArgs I{};
    uint64_t io = 0;
    uint32_t nout = 0;
    for (uint32_t q = 0; q < W; ++q) {
      const uint64_t nb = q == me ? 0 : hw[kRemoteWRecv + 2 * q];
      if (nb > (nreq[q] ? kRemoteHdr + (uint64_t)kRemoteDir * nreq[q] + asked[q] : 0)) {
        std::fprintf(stderr, "ripplemq: rank %u announced a repair response of %llu bytes\n", q, (unsigned long long)nb);
        return RMQ_EDEVICE;
      }
      x.peer(q, B.out + S.out_off[q], resp[q], nullptr, nb);
      I.in_off[q] = io;
      I.in_bytes[q] = nb;
      I.w0[q] = nout;
      io += pad16(nb);
      nout += nreq[q];
    }
    for (uint32_t q = W; q <= kMaxWorld; ++q) I.w0[q] = nout;
    rc = rr_grow(B, &B.in, &B.in_cap, std::max<uint64_t>(io, 16));
    if (rc) return rc;
    for (uint32_t q = 0; q < W; ++q) x.rb[q] = B.in + I.in_off[q];
    rc = x.post(r);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(B.ev, r->xchg_s));
    HIP_TRY(hipStreamWaitEvent(e->main_s, B.ev, 0));
    // 6. the install
    if (n && nout) {
      I.r = *a;
      I.want = B.want;
      I.lists = B.lists;
      I.list_cap = list_cap;
      I.in = B.in;
      I.fetched = B.fetched;
      I.world = W;
      launch_remote_install(I, e->main_s);
      HIP_TRY(hipGetLastError());
    }
    // (the next round's request kernel rewrites the lists and the next exchange the buffers: both
    // streams are waited for where the round's counters are read, the exchange stream here)
    HIP_TRY(hipStreamSynchronize(r->xchg_s));
  }
  HIP_TRY(hipStreamSynchronize(r->xchg_s));
  HIP_TRY(hipStreamSynchronize(e->main_s));
  if (n) HIP_TRY(hipMemcpy(fetched, B.fetched, 2ull * n * 8, hipMemcpyDeviceToHost));
  return RMQ_OK;
}

}  // namespace rmq
