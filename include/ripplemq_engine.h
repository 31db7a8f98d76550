/*
 * ripplemq_engine.h — C-ABI of the MI355X-native Partition-Raft engine.
 *
 * This is the drop-in boundary for RippleMQ's partition data path.
 * The Java broker keeps its RPC processors; each processor replaces the call it makes into
 * the per-partition jraft group with a call into this library (JNI stub: INTEGRATION.md).
 *
 * Reference interface each entry point replaces (paths relative to the reference root):
 *
 *   rmq_append                  <- Node.apply(new Task(ByteBuffer, done)) for a MessageAppendRequest,
 *                                  mq-broker/src/main/java/metadata/raft/request/processor/
 *                                  MessageAppendRequestProcessor.java:52-59, applied by
 *                                  PartitionStateMachine.onApply/handleMessageAppendRequest
 *                                  (mq-broker/src/main/java/metadata/raft/PartitionStateMachine.java:38-69)
 *   rmq_poll_commit             <- the PartitionClosure completion (request/PartitionClosure.java:32-36)
 *                                  that turns Status into MessageAppendResponse{success,errorMsg}
 *                                  (MessageAppendRequestProcessor.java:39-48); jraft BallotBox commit
 *   rmq_ack                     <- follower AppendEntries success -> BallotBox.commitAt  [jraft, SURVEY §3.4]
 *   rmq_commit_consumer_offset  <- Node.apply for a ConsumerOffsetUpdateRequest
 *                                  (ConsumerOffsetUpdateRequestProcessor.java:38-60) applied by
 *                                  PartitionStateMachine.handleConsumerOffsetUpdateRequest (:71-77)
 *   rmq_fetch                   <- PartitionStateMachine.handleBatchRead (:85-110) called from
 *                                  MessageBatchReadRequestProcessor.java:39 (direct read, no read-index)
 *   rmq_become_leader           <- PartitionStateMachine.onLeaderStart(term) (:121-126)
 *   rmq_vote / rmq_leader_silent <- jraft's RequestVote and election timer of each partition group
 *                                  (PartitionRaftServer.setupRaft: electionTimeoutMs 1000, raft_meta
 *                                  term/votedFor, PartitionRaftServer.java:85,89)  [jraft]
 *   rmq_set_replicas            <- PartitionRaftServer.setupRaft initial Configuration(peers)
 *                                  (mq-broker/src/main/java/metadata/raft/PartitionRaftServer.java:82-86)
 *   rmq_create / rmq_destroy    <- PartitionManager.startPartition / PartitionRaftServer.shutdown
 *                                  (PartitionManager.java:166-176, PartitionRaftServer.java:100-108)
 *   rmq_set_segments            <- no reference counterpart (its logs never evict, PartitionStateMachine.java
 *                                  :26,66): per-partition retention size inside a shared HBM pool
 *   rmq_set_placement           <- PartitionManager.handleTopicListChange starting the groups this broker
 *                                  hosts with their peers (PartitionManager.java:111-176), as placed by
 *                                  PartitionAssigner.assignPartitions (PartitionAssigner.java:25-94)
 *   rmq_attach_rccl /           <- the shared RpcServer/BoltRpcClient pair jraft replicates over
 *   rmq_attach_local               (PartitionRaftServer.java:93): AppendEntries to the followers and
 *                                  their acks, here grouped RCCL send/recv of replica-log rounds
 *                                  (FORMAT.md §9) between the engines of one node
 *
 * Only dense partition indices (pidx) cross this boundary; the Java side keeps the
 * "topic-partitionId" -> pidx map (PartitionManager.java:121,196-198).
 *
 * Threading: one submitter thread per engine for rmq_append / rmq_ack /
 * rmq_commit_consumer_offset / rmq_become_leader / rmq_set_replicas. rmq_fetch, rmq_poll_commit
 * and the read-back calls may be called from any thread (they serialize on an internal lock).
 * Completion is by polling tickets; the library never calls back into the host.
 *
 * Replication transport (multi-GPU): after rmq_attach_rccl / rmq_attach_local the
 * engines of the world replicate every launch group of appends to the followers named by the
 * placement and commit on quorum. Rounds are collective, like the launches that drive them: every
 * rank must make the same sequence of rmq_append calls (empty batches count) and of the calls that
 * flush the pipeline (rmq_sync, rmq_set_placement, rmq_set_replicas, rmq_become_leader, rmq_ack);
 * rmq_poll_commit / rmq_ticket_stats never flush then: they answer RMQ_PENDING until later launch
 * groups (further rmq_append calls on every rank, empty batches included: ripplemq_amd/pacer.py) or
 * an rmq_sync on every rank pushed the ticket through its stages; rmq_sync before rmq_destroy.
 *
 * Log byte format, offset index and retention are defined in FORMAT.md.
 */
#ifndef RIPPLEMQ_ENGINE_H
#define RIPPLEMQ_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMQ_ABI_VERSION 11u
#define RMQ_MAX_RF 8u
#define RMQ_ALL_PARTITIONS 0xFFFFFFFFu
#define RMQ_OFFSET_NONE 0xFFFFFFFFFFFFFFFFull /* out_offsets value of a rejected record */
#define RMQ_RECORD_HEADER_BYTES 16u
#define RMQ_RECORD_ALIGN 16u /* records start and end on 16-byte boundaries (FORMAT.md §1) */
#define RMQ_TICKET_OFFSETS 0x8000000000000000ull /* tickets of rmq_commit_consumer_offset carry this bit */

/* Status codes. Negative = error; RMQ_PENDING is a non-error poll result. */
enum {
  RMQ_OK = 0,
  RMQ_PENDING = 1,
  RMQ_ENOTLEADER = -1, /* "Not leader" reply of the reference processors */
  RMQ_ENOPART = -2,    /* unknown pidx (reference: NPE at MessageAppendRequestProcessor.java:29) */
  RMQ_EINVAL = -3,
  RMQ_ENOSPC = -4,     /* batch larger than configured capacity / fetch output buffer too small */
  RMQ_EDEVICE = -5,    /* HIP runtime error or no HIP device */
  RMQ_EOFFSET = -6,    /* fetch offset below the retained log start (evicted by retention) */
  RMQ_ENOMEM = -7,
  RMQ_ESTALE = -8,     /* rmq_become_leader: this replica lacks records its partition's leader
                          committed (Raft's vote restriction: it may not lead) */
  RMQ_ETERM = -9,      /* rmq_become_leader: the term already has a leader here (this replica led it,
                          or voted for another candidate in it: Raft's one vote per term) */
  RMQ_ECORRUPT = -10   /* ABI 11: a stored record fails its CRC32C or the log's structure (FORMAT.md §10):
                          rmq_scrub, and a fetch request with RMQ_FETCH_VERIFY */
};
#define RMQ_NO_VOTE 0xFFFFFFFFu /* rmq_partition_state.voted_for: no vote in voted_term */

/* Memory kind of caller buffers.
   RMQ_MEM_HOST: pageable host memory (rmq_append packs it into a pinned staging slot with host
     threads, then one DMA; payload ranges are checked on the host: RMQ_EINVAL).
   RMQ_MEM_DEVICE: device memory (rmq_device_alloc).
   RMQ_MEM_PINNED (rmq_append only): page-locked host memory (rmq_host_alloc, or pages registered
     with rmq_host_register): every section goes to the device by its own DMA on the engine's copy
     stream, with no host copy; out_offsets must be page-locked too and is written by a DMA. The
     caller keeps all of them unchanged until the ticket completes (like device batches), and
     payload ranges are checked on the device like device batches (rejected_invalid). */
enum { RMQ_MEM_HOST = 0, RMQ_MEM_DEVICE = 1, RMQ_MEM_PINNED = 2 };

typedef struct rmq_config {
  uint32_t num_partitions;     /* P: dense pidx in [0, P), P <= 65536 per engine */
  uint32_t replication_factor; /* RF in [1, RMQ_MAX_RF]; quorum = RF/2 + 1 */
  uint64_t segment_bytes;      /* ring bytes per (replica, partition) log; multiple of index_interval */
  uint32_t index_interval;     /* sparse offset-index interval in bytes; power of two in [64, 1<<20] */
  uint32_t max_consumers;      /* consumer-offset table width per partition (dense consumer ids) */
  uint32_t max_batch_records;  /* capacity of one rmq_append call */
  uint32_t pipeline_depth;     /* batches applied per pipeline launch group, 1..8; 0 -> default 2 */
  uint64_t max_batch_bytes;    /* payload bytes of one rmq_append call */
  int32_t device;              /* HIP device ordinal */
  uint32_t rank;               /* replica rank of this engine (placement in rmq_set_replicas) */
  uint64_t pool_bytes;         /* ring bytes per replica shared by all partitions (FORMAT.md §2);
                                  0 -> num_partitions * segment_bytes. Every partition starts with a
                                  segment_bytes ring; rmq_set_segments resizes them inside the pool */
} rmq_config;

/* One append batch: records of many partitions, interleaved, in apply order (SoA). */
typedef struct rmq_batch {
  uint32_t n;                  /* number of records */
  uint32_t mem;                /* RMQ_MEM_HOST, RMQ_MEM_DEVICE or RMQ_MEM_PINNED for every pointer below */
  const uint32_t* pidx;        /* [n] partition of each record */
  const uint32_t* len;         /* [n] payload length of each record */
  const uint64_t* payload_off; /* [n] byte offset of each payload in `payload`, or NULL = packed
                                  (payload_off[i] = sum of len[j], j < i) */
  const uint8_t* payload;      /* payload bytes */
  uint64_t payload_bytes;      /* readable bytes at `payload` */
} rmq_batch;

typedef struct rmq_fetch_req {
  uint32_t pidx;
  uint32_t consumer;           /* dense consumer id in [0, max_consumers) */
  uint32_t max_records;        /* reference: MessageBatchReadRequest.maxMessages */
  uint32_t flags;              /* RMQ_FETCH_COMMIT | RMQ_FETCH_REPLICA | RMQ_FETCH_VERIFY, or 0 */
} rmq_fetch_req;
/* rmq_fetch_req.flags: once the request is served (RMQ_OK, its records in the output) or answered
   RMQ_EOFFSET, commit the consumer's next offset — start_offset + count (the first retained offset
   for RMQ_EOFFSET) — as rmq_commit_consumer_offset would (no ticket; with a transport the row
   travels with the next round). The consumer client's read-then-commit
   (ConsumerClientImpl.java:61-117) in one device pass. At most one committing request per
   (partition, consumer) in a call (RMQ_EINVAL otherwise). */
#define RMQ_FETCH_COMMIT 1u
/* rmq_fetch_req.flags (ABI 10): read this engine's own replica of pidx, whether it leads the
   partition or follows it: the slice starts at the partition's replica cursor (rmq_set_replica_cursor;
   the consumer field only keys the position cache and must be < max_consumers) and ends at the
   replica's commit (its high_watermark: on a follower the part of its log below the leader commit
   it learned). With RMQ_FETCH_COMMIT the replica cursor moves to start_offset + count (local to this
   engine, never replicated; one committing replica request per partition in a call). This is how a
   replica's durable tier reads its own log: jraft keeps the whole log on every node
   (PartitionRaftServer.java:53,88-90), so a follower persists what it holds, not only a leader. */
#define RMQ_FETCH_REPLICA 2u
/* rmq_fetch_req.flags (ABI 11): once the request's slice is in the output, check every record of
   it as FORMAT.md §1 prescribes (header offsets start_offset, start_offset + 1, ..., records back to
   back filling `bytes` exactly, CRC32C of the payload, zero padding). A slice with a failing record
   is answered status RMQ_ECORRUPT and count 0; its start_offset, out_pos and bytes stay, so the
   caller sees what was refused and the out_pos of later requests do not move (a host output keeps
   its bytes of that range as they were). rmq_fetch / rmq_fetch_poll still return RMQ_OK or
   RMQ_ENOSPC: corruption is reported per request. With RMQ_FETCH_COMMIT a refused request commits
   nothing. Valid with RMQ_FETCH_REPLICA. Host rows only (device rows: flags 0, ignored). A call
   with such a request is never held back to go with later asynchronous fetches. (Bits 4, 8 and 16
   stay unknown flags, refused with RMQ_EINVAL as before.) */
#define RMQ_FETCH_VERIFY 0x20u

typedef struct rmq_fetch_res {
  uint64_t start_offset;       /* reference: MessageBatchReadResponse.offset (the consumer offset);
                                  RMQ_EOFFSET: the first retained offset, where the consumer can resume */
  uint64_t out_pos;            /* byte position of this request's records in the output buffer */
  uint32_t count;              /* records returned (reference: messages.size()) */
  uint32_t bytes;              /* bytes of the returned records (FORMAT.md record layout) */
  int32_t status;              /* RMQ_OK, RMQ_ENOTLEADER, RMQ_ENOPART, RMQ_EINVAL, RMQ_EOFFSET, RMQ_ENOSPC,
                                  RMQ_ECORRUPT (RMQ_FETCH_VERIFY) */
  uint32_t reserved;           /* 0, but rmq_fetch_bytes: a request whose first record exceeds its budget
                                  (status RMQ_ENOSPC) holds that record's size here */
} rmq_fetch_res;

typedef struct rmq_partition_state {
  uint64_t log_end_offset;     /* next offset to assign (reference: messages.size() on the leader) */
  uint64_t log_end_pos;        /* logical byte position of the log end */
  uint64_t log_start_offset;   /* first retained offset */
  uint64_t log_start_pos;      /* logical byte position of log_start_offset */
  uint64_t commit;             /* quorum commit (count of committed records) */
  uint64_t high_watermark;     /* consumer-visible end (== commit) */
  uint64_t term;
  uint64_t term_start;         /* log_end_offset at rmq_become_leader */
  uint64_t match[RMQ_MAX_RF];  /* per replica slot: records known persisted */
  uint32_t replica_rank[RMQ_MAX_RF];
  uint32_t leader_slot;
  uint32_t is_leader;
  uint64_t segment_bytes;      /* ring bytes of this partition (retention keeps at most this much) */
  uint64_t leader_commit;      /* the newest commit index of the partition's leader this replica knows
                                  (the Raft leaderCommit of the rounds and commit notices it received,
                                  FORMAT.md §9); on the leader its own commit. A replica whose log
                                  ends below it lacks committed records (rmq_become_leader: RMQ_ESTALE) */
  /* ABI 8: leader election (PartitionRaftServer.java:85,89) */
  uint64_t last_log_term;      /* Raft's lastLogTerm: the newest term whose leader-start entry this
                                  replica's log holds (its own term once it leads; on a follower the
                                  term of the last round entry it accepted that reached its leader's
                                  term start; 0 = unknown, after a catch-up that ended below its
                                  leader's term start: rmq_vote then compares against an upper bound,
                                  the leader's term - 1, while a candidacy claims 0) */
  uint64_t voted_term;         /* the term of this replica's last vote (raft_meta votedFor's term) */
  uint32_t voted_for;          /* the rank it voted for in voted_term (RMQ_NO_VOTE: none) */
  uint32_t led;                /* 1: this replica led voted_term (rmq_become_leader succeeded in it) */
  uint64_t heard_round;        /* the round stamp at which this replica last heard its partition's
                                  leader (a round entry or a commit notice of the current term);
                                  rmq_leader_silent compares it with the engine's round count */
} rmq_partition_state;

typedef struct rmq_append_stats {
  uint32_t records;            /* records submitted */
  uint32_t appended;           /* records given offsets */
  uint32_t rejected_not_leader;
  uint32_t rejected_no_partition;
  uint32_t rejected_no_space;  /* records of partitions whose record bytes in this batch exceed
                                  segment - interval (FORMAT.md §3: the partition takes none) */
  uint32_t rejected_invalid;   /* device batches only: whole batch rejected, a payload range lies
                                  outside payload_bytes (host batches get RMQ_EINVAL instead) */
} rmq_append_stats;

typedef struct rmq_repl_stats {
  uint32_t world, rank;
  uint32_t out_entries;        /* (led partition, remote slot) pairs this engine sends rounds for */
  uint32_t in_entries;         /* (followed partition, local slot) pairs it receives rounds for */
  uint64_t rounds;             /* replication rounds posted (one per launch group) */
  uint64_t bytes_sent;         /* round regions sent (FORMAT.md §9), all peers */
  uint64_t bytes_received;
  uint64_t records_ingested;   /* follower records whose CRC32C and log position checked out */
  uint64_t refused_crc;        /* follower entries refused: a record's CRC32C / header / bounds is wrong */
  uint64_t refused_log;        /* follower entries refused: do not continue the follower's log, stale
                                  leader term, or the round missed (no region from the leader) */
  uint64_t bytes_ingested;
  uint64_t catchup_entries;    /* leader: entries that re-sent a follower's gap (FORMAT.md §9 catch-up) */
  uint64_t detached_plans;     /* leader: entry plans whose follower lies beyond the ring and no rebase point was complete (FORMAT.md §9) */
  uint64_t general_plans;      /* leader: destination plans by the general path (a consumer-offset row or
                                  a catch-up gap among the entries, or over 4,096 entries); the
                                  steady-state plan covers the rest. A diagnostic of the round's cost */
  uint64_t host_waits;         /* rounds whose {bytes, records} swap had not landed when the host
                                  posted the round (RCCL's send/recv take host-side byte counts) */
  uint64_t host_wait_ns;       /* host time spent in those waits */
} rmq_repl_stats;

typedef struct rmq_engine rmq_engine;
typedef struct rmq_local_hub rmq_local_hub;

uint32_t rmq_abi_version(void);
const char* rmq_strerror(int status);
/* Fills a config with the defaults documented in DESIGN.md for P partitions and RF replicas. */
void rmq_config_default(rmq_config* cfg, uint32_t num_partitions, uint32_t replication_factor);

int rmq_create(const rmq_config* cfg, rmq_engine** out);
void rmq_destroy(rmq_engine* e);

/* Replica placement of one partition (reference: the Configuration(peers) of its raft group).
   replica_ranks[slot] = rank holding that replica; leader_slot names the leader replica.
   The engine leads pidx iff replica_ranks[leader_slot] == cfg.rank. rf must equal cfg RF. */
int rmq_set_replicas(rmq_engine* e, uint32_t pidx, const uint32_t* replica_ranks, uint32_t rf,
                     uint32_t leader_slot);
/* Placement of n partitions at once (one drain): for partition pidx[i], replica_ranks[i * RF + slot]
   and leader_slot[i] as in rmq_set_replicas, and key[i] (nullable: keys unchanged, default pidx) a
   cluster-wide id of the partition (its groupId) that orders replication lists identically on
   every rank (FORMAT.md §9). With a transport attached this is collective and checks every pair of
   ranks agrees on what they replicate to each other (RMQ_EINVAL on every rank if not). */
int rmq_set_placement(rmq_engine* e, uint32_t n, const uint32_t* pidx, const uint64_t* key,
                      const uint32_t* replica_ranks, const uint32_t* leader_slot);

/* Ring sizes of n partitions (reference: per-topic log retention; the reference keeps every
   message in memory, PartitionStateMachine.java:26,66): segment_bytes[i] (power of two, at least
   4 * index_interval) for partition pidx[i], allocated from the engine's pool. A shrinking ring
   first applies retention at the new size (FORMAT.md §4 rule); the retained records, their bytes in
   every local replica and their index entries keep their offsets and logical positions. All or
   nothing: RMQ_ENOMEM (nothing changed) if the pool cannot hold the new rings. Drains first (with a
   transport attached: collective, like rmq_sync). */
int rmq_set_segments(rmq_engine* e, uint32_t n, const uint32_t* pidx, const uint64_t* segment_bytes);

/* New leader term for pidx (or RMQ_ALL_PARTITIONS): term_start = log_end_offset, so only
   entries appended in this term can advance the commit (Raft current-term rule). */
int rmq_become_leader(rmq_engine* e, uint32_t pidx, uint64_t term);
/* Raft RequestVote on this replica (jraft's election, PartitionRaftServer.java:85; the vote persists
   in raft_meta, :89): a request of an older term is denied; a newer term is adopted first (a leader
   of pidx steps down: it stops accepting appends, offset commits and fetches); the vote is granted
   when this replica has not voted for another candidate in `term` and the candidate's log is at least
   as up to date, (cand_last_log_term, cand_log_end) >= (last_log_term, log_end_offset) in that order.
   *granted = 1 records the vote (voted_term = term, voted_for = candidate). A candidate votes for
   itself through this call too, then rmq_become_leader(pidx, term) once a quorum granted.
   Without a transport the batches submitted are applied first. With one nothing is flushed (a flush
   is collective): the call waits for what is issued only, and a replica that leads pidx with launch
   groups still in flight answers RMQ_PENDING with nothing changed (the request is delayed: send it
   again after the next rmq_sync). */
int rmq_vote(rmq_engine* e, uint32_t pidx, uint64_t term, uint32_t candidate, uint64_t cand_last_log_term,
             uint64_t cand_log_end, uint32_t* granted);
/* Replay of a persisted vote (raft_meta): voted_term / voted_for of pidx, and the term if newer. */
int rmq_set_vote(rmq_engine* e, uint32_t pidx, uint64_t term, uint32_t voted_for);
/* Partitions this replica follows whose leader has been silent (jraft's election timeout, 1000 ms,
   PartitionRaftServer.java:85): no round entry or commit notice of the current term from the leader
   in the last `silent_rounds` rounds (heard_round + silent_rounds <= the engine's round count) AND
   none for at least timeout_ms of wall time. out_pidx gets at most cap of them in ascending order,
   *n = how many there are. A placement change restarts every partition's timer. */
int rmq_leader_silent(rmq_engine* e, uint32_t silent_rounds, uint32_t timeout_ms, uint32_t* out_pidx,
                      uint32_t cap, uint32_t* n);

/* Append one batch. Assigns offsets (stable per partition, in batch order), writes the records
   with CRC32C into every local replica log, advances the offset index, the quorum commit and
   the high watermark. Asynchronous: returns a ticket; caller buffers must stay valid until
   rmq_poll_commit(ticket) returns RMQ_OK. out_offsets (same memory kind as the batch) gets the
   offset of each record, or RMQ_OFFSET_NONE if it was rejected (unknown pidx / not leader / no
   space). A partition whose record bytes in this batch (sum of 16 + align16(len)) exceed
   segment_bytes - index_interval takes none of the batch's records (rmq_ticket_stats reports them
   as rejected_no_space); the batch's other partitions are unaffected.
   Batches are collected into launch groups of up to cfg.pipeline_depth: the call that fills a
   group issues one kernel launch that ranks it and advances the three groups submitted before
   it (scan, apply, retention); every batch keeps its own semantics. A batch is applied by the
   second launch after its group's own, or when rmq_poll_commit / rmq_ticket_stats / rmq_sync /
   any control call closes the forming group and flushes the pipeline. */
int rmq_append(rmq_engine* e, const rmq_batch* batch, uint64_t* out_offsets, uint64_t* ticket);

/* External replica acks (followers on other ranks): match[slot] = max(match[slot],
   min(value, log_end_offset)),
   then the quorum commit rule is re-evaluated for those partitions. Host arrays of n. */
int rmq_ack(rmq_engine* e, const uint32_t* pidx, const uint32_t* replica_slot,
            const uint64_t* match, uint32_t n);

/* Append tickets: RMQ_OK if every operation up to `ticket` completed (then commit/hw snapshots of all
   P partitions are copied to the optional host arrays), RMQ_PENDING if not yet.
   Consumer-offset tickets (RMQ_TICKET_OFFSETS set, from rmq_commit_consumer_offset): RMQ_OK once the
   consumer-offset row of every partition the call committed to, as of that call or newer, is held
   by a quorum of the partition's replicas (co-located replicas hold it once applied; a remote one
   once it accepted a round carrying it, FORMAT.md §8) — the reference's PartitionClosure answering a
   ConsumerOffsetUpdateRequest after the Raft commit (ConsumerOffsetUpdateRequestProcessor.java:40-49,
   60, PartitionClosure.java:32-36); RMQ_PENDING until then; RMQ_ENOTLEADER if this engine stopped
   leading one of those partitions first (the commit may be lost, like a jraft closure failed by a
   leader change). A resolved offset ticket is forgotten (a second poll: RMQ_EINVAL). Never flushes. */
int rmq_poll_commit(rmq_engine* e, uint64_t ticket, uint64_t* commit_out, uint64_t* hw_out);
int rmq_ticket_stats(rmq_engine* e, uint64_t ticket, rmq_append_stats* out);
int rmq_sync(rmq_engine* e);

/* Consumer-offset commits, applied in array order: last writer wins, no bounds or monotonic
   check (PartitionStateMachine.java:71-77). status (nullable, host, [n]) reports per item (not
   leader, unknown partition, bad consumer id). The items reach the device table in order with the
   append stream (one copy on the pipeline stream, no wait for the pipeline): a later rmq_fetch or
   read-back sees them. With a replication transport the partition's row travels to every follower
   with the next round (FORMAT.md §8, §9). ticket (nullable) gets a consumer-offset ticket
   (RMQ_TICKET_OFFSETS set) that rmq_poll_commit resolves once the accepted items are on a quorum;
   0 if no item was accepted. The engine keeps the 256 newest unpolled offset tickets: an older
   one polls as RMQ_EINVAL. */
int rmq_commit_consumer_offset(rmq_engine* e, const uint32_t* pidx, const uint32_t* consumer,
                               const uint64_t* offset, uint32_t n, int32_t* status, uint64_t* ticket);
/* ABI 10: the replica cursors of n partitions (where RMQ_FETCH_REPLICA reads start): a durable
   tier's end after it reopens its files. Local to this engine (no round carries it); ordered with
   the pipeline stream like a consumer-offset commit. */
int rmq_set_replica_cursor(rmq_engine* e, uint32_t n, const uint32_t* pidx, const uint64_t* offset);

/* Batched consumer fetch: for each request, off = committed consumer offset (default 0),
   returns records [off, min(off + max, high_watermark)) (PartitionStateMachine.java:85-110).
   Records are copied in FORMAT.md layout, request after request, into `out` (mem kind `mem`).
   reqs/res are host arrays. Synchronous. Returns RMQ_OK, or RMQ_ENOSPC if some request did not
   fit in out_cap (those get count 0, status RMQ_ENOSPC). */
int rmq_fetch(rmq_engine* e, const rmq_fetch_req* reqs, uint32_t n, uint32_t mem, uint8_t* out,
              uint64_t out_cap, rmq_fetch_res* res, uint64_t* bytes_used);
/* rmq_fetch without blocking the host (ABI 6). The fetch is ordered after every launch and call
   issued before it and before the ones issued after it, exactly like rmq_fetch, and returns at once
   with a fetch ticket; reqs are copied before the call returns. res (and out with RMQ_MEM_HOST)
   must stay valid until rmq_fetch_poll returns something other than RMQ_PENDING. Four fetches can
   be in flight: a fifth first completes the oldest into its caller's arrays (its poll then returns
   at once). MessageBatchReadRequestProcessor.java:36-42 answers each read from its own closure;
   this is the batched, pipelined form of that call.
   mem | RMQ_FETCH_PINNED_ROWS (ABI 7; rmq_fetch too): reqs and res are page-locked host memory
   (rmq_host_alloc or rmq_host_register): the fetch kernels read the request rows and write the
   result rows there themselves, with no copy (rows the runtime cannot map are staged like ordinary
   ones). The caller then keeps reqs unchanged until the ticket completes (as with pinned batches);
   res is written before the poll that returns the result.
   mem | RMQ_FETCH_DEVICE_ROWS (ABI 9; rmq_fetch too): reqs and res are device memory (a broker whose
   requests arrive on the GPU): no transfer at all. The host never sees these requests, so their
   flags word must be 0 (RMQ_FETCH_COMMIT needs host rows: the call checks them) and is ignored.
   mem | RMQ_FETCH_FILL (added after ABI 11 without a version bump; every fetch entry point, with
   ordinary, pinned or device rows; FORMAT.md §7 "Filling a bounded output"; a Kafka fetch request's
   fetch.max.bytes): out_cap bounds the whole call instead of failing it. Answer the call with an
   unlimited out_cap (budgets and explicit offsets applied): row r has B_r bytes, P_r before it. If
   everything fits out_cap, the call is answered exactly as without the flag. Otherwise, with r* the
   first request with P_r + B_r > out_cap: the requests before r* are unchanged; r* is answered as
   rmq_fetch_bytes answers a budget of out_cap - P_r* (cut at the last record boundary inside it;
   count, bytes, commit and verify follow the cut; if not even its first record fits: count 0,
   bytes 0, nothing committed, that record's size in `reserved`, status RMQ_ENOSPC when P_r* = 0,
   the output itself being too small, else RMQ_PENDING); every later request that would have been
   served bytes is status RMQ_PENDING, start_offset as resolved, count 0, bytes 0, reserved 0: it
   takes no output and commits nothing (ask again); later rows without bytes (empty, RMQ_EOFFSET,
   errors, budget RMQ_ENOSPC) are unchanged. out_pos is the running sum of the final bytes,
   bytes_used <= out_cap, and the call returns RMQ_OK: no row is answered RMQ_ENOSPC for capacity.
   out == NULL with out_cap == 0 names the first record's size of the first request with records
   (RMQ_ENOSPC, `reserved`). Requests are served in request order: a caller that rotates its order
   from call to call is fair to all. A filling call is never held back to go with later
   asynchronous fetches. */
#define RMQ_FETCH_PINNED_ROWS 0x100u
#define RMQ_FETCH_DEVICE_ROWS 0x200u
#define RMQ_FETCH_FILL 0x400u
int rmq_fetch_async(rmq_engine* e, const rmq_fetch_req* reqs, uint32_t n, uint32_t mem, uint8_t* out,
                    uint64_t out_cap, rmq_fetch_res* res, uint64_t* ticket);
/* Completion of an rmq_fetch_async ticket: RMQ_PENDING while it runs (wait != 0: block instead), else
   what rmq_fetch would have returned (RMQ_OK / RMQ_ENOSPC) with res, out and *bytes_used filled. A
   ticket is answered once; an unknown or already answered ticket gets RMQ_EINVAL. */
int rmq_fetch_poll(rmq_engine* e, uint64_t ticket, uint32_t wait, uint64_t* bytes_used);
/* rmq_fetch / rmq_fetch_async with a byte budget per request (FORMAT.md §7 "Byte budgets"; added
   after ABI 11 without a version bump; a Kafka client's max.partition.fetch.bytes). max_bytes[r] is
   request r's budget in bytes of record images, 0: none; max_bytes == NULL is exactly rmq_fetch /
   rmq_fetch_async. A request that would be served more bytes than its budget is answered in every
   respect as if its max_records had been k*, the largest number of its records whose bytes are at
   most the budget (count, bytes, later requests' out_pos, the RMQ_ENOSPC test against out_cap,
   bytes_used, RMQ_FETCH_COMMIT, RMQ_FETCH_VERIFY, RMQ_FETCH_REPLICA). If even its first record
   exceeds the budget (k* = 0) its row is status RMQ_ENOSPC, count 0, bytes 0, with the first
   record's size in `reserved` (the budget that would serve it): it takes no output, commits
   nothing, and the call still returns RMQ_OK (reported per request, as RMQ_ECORRUPT is). A request
   that does not fit out_cap keeps reserved = 0. Empty slices, RMQ_EOFFSET and error rows are
   answered as without budgets. With host rows (ordinary or RMQ_FETCH_PINNED_ROWS) max_bytes is
   ordinary host memory, read before the call returns; with RMQ_FETCH_DEVICE_ROWS it is device
   memory, 4-byte aligned, valid until the ticket completes. A call with budgets is never held back
   to go with later asynchronous fetches. rmq_fetch_poll completes both kinds of ticket. */
int rmq_fetch_bytes(rmq_engine* e, const rmq_fetch_req* reqs, const uint32_t* max_bytes, uint32_t n,
                    uint32_t mem, uint8_t* out, uint64_t out_cap, rmq_fetch_res* res, uint64_t* bytes_used);
int rmq_fetch_bytes_async(rmq_engine* e, const rmq_fetch_req* reqs, const uint32_t* max_bytes, uint32_t n,
                          uint32_t mem, uint8_t* out, uint64_t out_cap, rmq_fetch_res* res, uint64_t* ticket);
/* rmq_fetch_bytes / rmq_fetch_bytes_async with an explicit start offset per request (FORMAT.md §7
   "Explicit offsets"; added after ABI 11 without a version bump; the fetch offset of a Kafka fetch
   request). offsets[r] == RMQ_OFFSET_NONE: request r is answered as ever, from its consumer's
   committed offset (or the replica cursor with RMQ_FETCH_REPLICA); any other value is the request's
   `off` instead, and the request is answered in every respect as if the committed offset (the
   replica cursor) had been that value when the call was ordered: an offset at or past the high
   watermark gives an empty RMQ_OK row with start_offset = off, one before the log start
   RMQ_EOFFSET with the first retained offset; max_records, byte budgets, out_pos, the RMQ_ENOSPC
   test, bytes_used and RMQ_FETCH_VERIFY as without it. Offset 2^64 - 1 itself cannot be asked for
   (a slice there is always empty). Nothing is written without RMQ_FETCH_COMMIT: neither the
   consumer table nor the replica cursor moves, and no round carries anything; with it the request
   commits start_offset + count (the first retained offset after RMQ_EOFFSET), a seek and a read
   in one call. A call may hold several non-committing requests of one (partition, consumer), at
   most one committing one. `consumer` must still be below max_consumers: it keys the position
   cache, which explicit requests consult and update like any other, and names the row a commit
   writes. offsets == NULL is exactly rmq_fetch_bytes / rmq_fetch_bytes_async (with max_bytes ==
   NULL too: rmq_fetch / rmq_fetch_async). With host rows (ordinary or RMQ_FETCH_PINNED_ROWS)
   offsets is ordinary host memory, read before the call returns; with RMQ_FETCH_DEVICE_ROWS it is
   device memory, 8-byte aligned (RMQ_EINVAL otherwise), valid until the ticket completes. A call
   with offsets is never held back to go with later asynchronous fetches. rmq_fetch_poll completes
   these tickets too. */
int rmq_fetch_at(rmq_engine* e, const rmq_fetch_req* reqs, const uint64_t* offsets, const uint32_t* max_bytes,
                 uint32_t n, uint32_t mem, uint8_t* out, uint64_t out_cap, rmq_fetch_res* res, uint64_t* bytes_used);
int rmq_fetch_at_async(rmq_engine* e, const rmq_fetch_req* reqs, const uint64_t* offsets, const uint32_t* max_bytes,
                       uint32_t n, uint32_t mem, uint8_t* out, uint64_t out_cap, rmq_fetch_res* res, uint64_t* ticket);
/* rmq_fetch_at / rmq_fetch_at_async with a per-record position table (FORMAT.md §7 "Record table";
   added after ABI 11 without a version bump; a Kafka fetch response is indexable by record, a run of
   record images is a chain of length words). Everything rmq_fetch_at takes, with the same meaning
   (offsets / max_bytes nullable, every `mem` bit, every request flag), and the call is answered as
   rmq_fetch_at answers it: rows, output bytes, bytes_used, commits and the position cache are the
   same bit for bit. One device pass after the gather (and the verify) then looks at the final rows:
   row r owns w_r = count_r + 1 table words if its status is RMQ_OK and count_r > 0, else none (empty
   rows, RMQ_EOFFSET, error rows, both kinds of RMQ_ENOSPC, RMQ_PENDING, RMQ_ECORRUPT).
   rec_row[r] = w_0 + ... + w_{r-1} for r in [0, n] (n + 1 words; rec_row[n] = the words the call
   needs). For an owning row rec_pos[rec_row[r] + k], k in [0, count_r), is the byte position of its
   record k inside its run out[out_pos_r, out_pos_r + bytes_r) (word 0 is 0), and
   rec_pos[rec_row[r] + count_r] = bytes_r: word for word what rmq_scan_records writes as pos_out for
   that run and what rmq_restore_item.table_start points at. A row's words are written only if
   rec_row[r] + w_r <= rec_cap; other words of rec_pos are left as they were. rec_row[n] > rec_cap
   returns RMQ_ENOSPC (from the call or the poll), with RMQ_FETCH_FILL too: the one way a filling
   call returns it; the caller tells the overflows apart by bytes_used > out_cap versus
   rec_row[n] > rec_cap. rec_cap >= out_cap / 16 + n always suffices (a record is at least 16
   bytes). rec_row == NULL, rec_pos == NULL, rec_cap == 0 is exactly rmq_fetch_at; rec_pos == NULL
   needs rec_cap == 0 and is a size probe (rec_row is written); rec_row == NULL with anything else,
   or rec_pos == NULL with rec_cap != 0, is RMQ_EINVAL. Both arrays have the memory kind of `out`
   (mem & 3): RMQ_MEM_HOST: ordinary host arrays, valid until the ticket completes, staged in slot
   scratch and copied back with the output bytes; RMQ_MEM_DEVICE: device memory, 8-byte aligned
   (RMQ_EINVAL otherwise), written in place. The words come from length words that nothing has
   checked unless the request carries RMQ_FETCH_VERIFY (a refused request owns no words): on an
   intact log they are the true record starts; on a damaged length word of an unflagged request they
   are still bounded: every word a multiple of 16 in [0, bytes_r], word 0 = 0, word count_r =
   bytes_r (q_0 = 0, q_{k+1} = min(q_k + 16 + align16(len at q_k), bytes_r) in 64-bit; once a q_k
   reaches bytes_r the words left are bytes_r), no byte outside the run is read and no word outside
   the row's own is written. A call with a table is never held back to go with later asynchronous
   fetches; rmq_fetch_poll completes these tickets too. */
int rmq_fetch_table(rmq_engine* e, const rmq_fetch_req* reqs, const uint64_t* offsets, const uint32_t* max_bytes,
                    uint32_t n, uint32_t mem, uint8_t* out, uint64_t out_cap, rmq_fetch_res* res,
                    uint64_t* rec_row, uint64_t* rec_pos, uint64_t rec_cap, uint64_t* bytes_used);
int rmq_fetch_table_async(rmq_engine* e, const rmq_fetch_req* reqs, const uint64_t* offsets, const uint32_t* max_bytes,
                          uint32_t n, uint32_t mem, uint8_t* out, uint64_t out_cap, rmq_fetch_res* res,
                          uint64_t* rec_row, uint64_t* rec_pos, uint64_t rec_cap, uint64_t* ticket);

/* ---- lag (added after ABI 11 without a bump, as the repairs were: one struct and one function,
   nothing existing moves) ---- */
typedef struct rmq_lag_res {   /* 64 bytes */
  uint64_t start_offset; /* where a fetch of this row would start: off; RMQ_EOFFSET: the first retained offset */
  uint64_t records;      /* records in [start_offset, high_watermark); 0 if off >= high_watermark */
  uint64_t bytes;        /* their record bytes: end_pos - start_pos */
  uint64_t evicted;      /* RMQ_EOFFSET: log_start_offset - off, records retention took before they were read; else 0 */
  uint64_t start_pos;    /* logical position (FORMAT.md §2) of record start_offset; 0 if records == 0 */
  uint64_t end_pos;      /* logical position of record high_watermark (log_end_pos when hw == log_end_offset); 0 if records == 0 */
  uint64_t headroom;     /* record bytes the partition can still take before retention evicts record start_offset
                            (below); RMQ_OFFSET_NONE if records == 0 */
  int32_t status;        /* RMQ_OK, RMQ_EOFFSET, RMQ_ENOTLEADER, RMQ_ENOPART, RMQ_EINVAL */
  uint32_t reserved;     /* 0 */
} rmq_lag_res;
/* How far behind a reader is, and how long it has (FORMAT.md §7 "Lag"; a Kafka consumer group's lag,
   in records and bytes, and the distance to retention). The rows are rmq_fetch_req rows, so a caller
   builds its rows once, asks for their lag and then fetches them. Row r, every word of its partition
   read in one pass of one kernel: the checks of a fetch in its order (pidx >= P: RMQ_ENOPART; a
   partition not led, without RMQ_FETCH_REPLICA: RMQ_ENOTLEADER; consumer >= max_consumers: RMQ_EINVAL;
   such a row is all 0 but headroom = RMQ_OFFSET_NONE). off is offsets[r] if offsets != NULL and the
   word is not RMQ_OFFSET_NONE, else the consumer's committed offset (the replica cursor with
   RMQ_FETCH_REPLICA): what rmq_fetch_at takes as off. end = high_watermark (with RMQ_FETCH_REPLICA
   this replica's own). off >= end: RMQ_OK, start_offset = off, every count and position 0, headroom =
   RMQ_OFFSET_NONE. Otherwise off < log_start_offset gives RMQ_EOFFSET with start_offset =
   log_start_offset and evicted = log_start_offset - off, else RMQ_OK with start_offset = off;
   records = end - start_offset (a high watermark at or below the log start: 0, with bytes, both
   positions 0 and headroom RMQ_OFFSET_NONE; status, start_offset and evicted stay); start_pos and
   end_pos by FORMAT.md §5's lookup; bytes = end_pos - start_pos, all 64-bit. headroom =
   max(floor(start_pos / index_interval) * index_interval, log_start_pos) + ring bytes - log_end_pos
   (0 for a state with more than the ring's bytes retained): record start_offset survives every
   sequence of appends to the partition whose record bytes total at most headroom, and from the
   present state one batch that carries 16 bytes more evicts it (where FORMAT.md §3 allows the batch).
   max_records is not read; RMQ_FETCH_REPLICA is honoured; RMQ_FETCH_COMMIT and RMQ_FETCH_VERIFY are
   accepted and do nothing (the call never commits, copies or verifies, and any number of rows may
   name one consumer); any other flag bit of a host row fails the call (RMQ_EINVAL) before anything
   runs; of a device row only the replica bit is looked at.
   mem is RMQ_MEM_HOST (reqs, offsets, res ordinary host arrays, staged through page-locked scratch
   of the call's own: no fetch slot is taken and no fetch ticket retired) or RMQ_MEM_DEVICE (reqs and
   res 16-byte aligned, offsets 8-byte aligned, RMQ_EINVAL otherwise; used in place); anything else,
   any RMQ_FETCH_* bit included, is RMQ_EINVAL, and so are a null engine and n != 0 with null reqs or
   res; n == 0 returns RMQ_OK and touches nothing; the argument checks come before any device call.
   Synchronous, from any thread. Ordered as rmq_fetch is: its kernel goes to the pipeline stream after
   every launch and call issued before it and before those issued after it, and the call waits for
   that kernel alone; it never flushes the forming group, never drains, is not collective with a
   transport, and writes nothing of the engine (no consumer row, cursor, position-cache entry or
   round). Returns RMQ_OK with per-row statuses, or RMQ_EINVAL, RMQ_ENOMEM, RMQ_EDEVICE. */
int rmq_lag(rmq_engine* e, const rmq_fetch_req* reqs, const uint64_t* offsets, uint32_t n, uint32_t mem,
            rmq_lag_res* res);

/* ---- record columns (added after ABI 11 without a bump, as rmq_lag was: two structs and one
   function, nothing existing moves) ---- */
typedef struct rmq_unpack_args {
  /* input: the answer of a COMPLETED rmq_fetch_table call with a device output */
  const uint8_t* buf;        /* the fetch's `out`, device memory, 16-byte aligned */
  uint64_t buf_bytes;        /* readable bytes at buf (its out_cap or bytes_used) */
  const rmq_fetch_res* rows; /* [n] its result rows: host memory, or device with RMQ_FETCH_DEVICE_ROWS in mem */
  const uint64_t* rec_row;   /* [n + 1] device, 8-byte aligned */
  const uint64_t* rec_pos;   /* [rec_words] device, 8-byte aligned */
  uint64_t rec_words;
  const uint32_t* row_tag;   /* [n] device, nullable: tag[j] of row r's records = row_tag[r], else r */
  /* output, all device memory */
  uint64_t* rec_first;       /* [n + 1] required: index of row r's first record in the columns; [n] = R */
  uint64_t* offset;          /* [rec_cap] nullable: header offset of record j */
  uint32_t* len;             /* [rec_cap] payload length of record j */
  uint64_t* payload_off;     /* [rec_cap] where record j's payload starts (below) */
  uint32_t* tag;             /* [rec_cap] nullable */
  uint64_t rec_cap;
  uint8_t* payload;          /* nullable: NULL = view mode */
  uint64_t payload_cap;
  uint32_t n, stride, mem, flags; /* flags 0 */
} rmq_unpack_args;
typedef struct rmq_unpack_res {  /* 48 bytes */
  uint64_t records;        /* R */
  uint64_t payload_bytes;  /* bytes the payload area needs: view 0, packed sum(len), strided R * stride */
  uint64_t mismatched;     /* records whose length word disagrees with their table extent */
  uint64_t truncated;      /* strided: records with len > stride */
  uint64_t bad_row;        /* lowest row that fails the structure checks; RMQ_OFFSET_NONE if none */
  int32_t status; uint32_t reserved;
} rmq_unpack_res;
/* The answer of a table fetch as columns (FORMAT.md §7 "Record columns"): what a device consumer
   computes on and what rmq_append takes, made on the device. Row r owns records iff its status is
   RMQ_OK and count_r > 0 (rmq_fetch_table's rule); record k of it, k in [0, count_r), is the image
   buf[out_pos_r + rec_pos[rec_row[r] + k], out_pos_r + rec_pos[rec_row[r] + k + 1]). rec_first[r] =
   the sum of count over the owning rows before r, R = rec_first[n]. Record j = rec_first[r] + k gets
   offset[j] = the header's offset word, tag[j] = row_tag[r] (r without row_tag), len[j] =
   min(header len, extent - 16); a record with 16 + align16(header len) != extent counts in
   `mismatched` (an unverified fetch over a damaged length word: the table's own trust level; fetch
   with RMQ_FETCH_VERIFY for integrity). Three modes. View (payload == NULL, which needs stride == 0
   and payload_cap == 0): payload_off[j] = out_pos_r + rec_pos[...] + 16, a byte offset into buf; no
   byte is copied and {n = R, pidx = tag, len, payload_off, payload = buf, payload_bytes = buf_bytes}
   is an rmq_batch of RMQ_MEM_DEVICE as it stands. Packed (payload != NULL, stride == 0):
   payload_off[j] = len[0] + ... + len[j - 1], the payloads back to back; payload_bytes = sum(len).
   Strided (stride > 0): payload_off[j] = j * stride; the first min(len[j], stride) payload bytes are
   copied and the rest of the slot is zero, len[j] stays the full length, records with len > stride
   count in `truncated`; payload_bytes = R * stride.
   Every table word, length word and position is checked on the device before it is an address, as
   rmq_restore checks its table. rec_row is non-decreasing with rec_row[n] <= rec_words; every row's
   word count is the table rule's (count_r + 1, or 0); an owning row has out_pos_r a multiple of 16,
   out_pos_r + bytes_r <= buf_bytes and count_r <= bytes_r / 16; its words start at 0, are multiples
   of 16, increase by at least 16 and end at bytes_r. A row that fails any of these fails the call:
   status and the return value are RMQ_EINVAL, bad_row is the lowest failing row, no column word and
   no payload byte is written (rec_first may be), no byte outside buf[0, buf_bytes) and no word
   outside the caller's arrays is read or written. R > rec_cap, or payload_bytes > payload_cap with a
   payload area, returns RMQ_ENOSPC: rec_first and `out` are written in full (size the arrays from
   them), no column word and no payload byte is. len == payload_off == NULL with rec_cap == 0 is the
   size probe (a packed probe passes any non-null payload with payload_cap 0).
   Checked before any device call, RMQ_EINVAL: a null engine, args or out; mem other than
   RMQ_MEM_DEVICE or RMQ_MEM_DEVICE | RMQ_FETCH_DEVICE_ROWS; nonzero flags; a misaligned pointer (buf
   and device rows 16, 64-bit arrays 8, 32-bit arrays 4; payload any); with n != 0 a null rows,
   rec_row or rec_first, a null rec_pos with rec_words != 0, a null buf with buf_bytes != 0, a null
   len or payload_off with rec_cap != 0; payload == NULL with a stride or a payload_cap. n == 0
   returns RMQ_OK with R = 0 and touches nothing but `out`, and rec_first[0] if rec_first is given.
   Host rows are staged through page-locked scratch of the call's own. Synchronous, from any thread.
   Ordered as rmq_lag is: its kernels go to the pipeline stream after every launch and call issued
   before it and before those issued after it, and the call waits for them alone; it never flushes
   the forming group, never drains, takes no fetch slot, is not collective with a transport and
   writes nothing of the engine. Returns RMQ_OK, RMQ_ENOSPC, RMQ_EINVAL, RMQ_ENOMEM or RMQ_EDEVICE;
   `out` is written whenever the argument checks pass. */
int rmq_unpack(rmq_engine* e, const rmq_unpack_args* a, rmq_unpack_res* out);

/* ---- replication transport (FORMAT.md §9) ---- */
/* 128-byte communicator id: one rank creates it, the application hands it to every rank. */
int rmq_rccl_unique_id(uint8_t* out /* 128 bytes */);
/* RCCL over xGMI between the world's engines, one per GPU and process; rank = cfg.rank. Collective. */
int rmq_attach_rccl(rmq_engine* e, const uint8_t* comm_id, uint32_t world);
/* In-process transport: engines of one process exchange by device copies; each rank's engine must
   be driven by its own host thread (the hub's barriers stand in for the collective). */
int rmq_local_hub_create(uint32_t world, rmq_local_hub** out);
void rmq_local_hub_destroy(rmq_local_hub* hub);
int rmq_attach_local(rmq_engine* e, rmq_local_hub* hub);
int rmq_replication_stats(rmq_engine* e, rmq_repl_stats* out);
/* Region bytes of the last posted round for destination rank dst (FORMAT.md §9): *size gets its
   length; copied to out if out != NULL and cap suffices (tests, tools). */
int rmq_read_outbox(rmq_engine* e, uint32_t dst, uint8_t* out, uint64_t cap, uint64_t* size);
/* Fault injection (tests): the rounds of the next n launch groups this engine forms from batches
   appended after the call send empty regions, as if the leader failed before replicating them
   (its own log keeps the records; followers neither see nor ack them). Not collective. */
int rmq_fault_drop_rounds(rmq_engine* e, uint32_t n);
/* Fault injection (tests): the regions of the next n rounds this engine sends to rank dst are lost
   (launch groups formed from batches appended after the call), as a failed link to dst would lose
   them: dst misses those rounds (every entry refused); its other peers and the commit notices of a
   drain still reach it. Not collective. */
int rmq_fault_isolate(rmq_engine* e, uint32_t dst, uint32_t n);
/* Fault injection (tests): as rmq_fault_isolate, and the commit notices of the next drain to dst are
   lost as well: a network partition between this leader and dst (dst's rmq_leader_silent reports the
   partitions this engine leads toward it). Not collective. */
int rmq_fault_cut(rmq_engine* e, uint32_t dst, uint32_t n);
/* Fault injection (tests): the next round this engine sends to rank dst has the byte at `at` of its
   region XORed with 0x5A (at < 0: counted back from the end of the region's data section, i.e. a
   payload byte of its last record), as a link or memory corruption would; the follower refuses the
   entry it hits and the leader's catch-up re-sends it (FORMAT.md §9). Not collective. */
int rmq_fault_corrupt(rmq_engine* e, uint32_t dst, int64_t at);

/* ---- read-back (tests, tools) ---- */
int rmq_get_partition_state(rmq_engine* e, uint32_t pidx, rmq_partition_state* out);
/* The states of partitions [first, first + n) at once (one device copy per field). */
int rmq_get_partition_states(rmq_engine* e, uint32_t first, uint32_t n, rmq_partition_state* out);
/* Raw ring bytes [ring_off, ring_off + len) of replica slot `replica` of pidx. */
int rmq_read_segment(rmq_engine* e, uint32_t replica, uint32_t pidx, uint64_t ring_off,
                     uint64_t len, uint8_t* out);
/* Offset-index entries m in [m_first, m_first + count): out[2k] = offset, out[2k+1] = pos. */
int rmq_read_index(rmq_engine* e, uint32_t pidx, uint64_t m_first, uint64_t count, uint64_t* out);
int rmq_read_consumer_offsets(rmq_engine* e, uint32_t pidx, uint64_t* out /* max_consumers */);
/* The consumer-offset rows of partitions [first, first + n): out[n][max_consumers]. */
int rmq_read_consumer_table(rmq_engine* e, uint32_t first, uint32_t n, uint64_t* out);

/* ---- scrub (ABI 11, FORMAT.md §10) ---- */
#define RMQ_SCRUB_BAD_CRC   1u  /* CRC32C of the payload differs from the header's, or a padding byte is not zero */
#define RMQ_SCRUB_BAD_CHAIN 2u  /* header offset is not the expected one, the record runs past its segment's end,
                                   or the walk from an index entry does not land on the next entry / the log end */
typedef struct rmq_scrub_res {
  uint64_t records_ok;   /* records that passed, summed over the local replicas checked */
  uint64_t bytes_ok;     /* their record bytes (16 + align16(len)) */
  uint64_t bad_offset;   /* lowest expected offset of a failing record; RMQ_OFFSET_NONE if none */
  uint32_t bad_replica;  /* lowest replica slot on which that offset fails */
  uint32_t bad_kind;     /* RMQ_SCRUB_BAD_* of that (offset, replica) */
  uint32_t replicas;     /* local replica slots checked (0: this engine holds no replica of the partition) */
  int32_t status;        /* RMQ_OK or RMQ_ECORRUPT */
} rmq_scrub_res;
/* On-device audit of the retained logs [log_start_offset, log_end_offset) of every local replica
   slot of partitions [first, first + n), led or followed: every record's header offset, extent,
   CRC32C and zero padding, and the sparse index entries that tile the log (FORMAT.md §10). res
   (host, [n], nullable) gets one row per partition. Returns RMQ_OK if every partition is clean,
   RMQ_ECORRUPT if any is not (the rows say where), RMQ_ENOPART if the range leaves [0, P). Changes no
   engine state. Drains first, like rmq_sync: with a transport attached the call is collective (every
   rank makes it at the same point of its call sequence). */
int rmq_scrub(rmq_engine* e, uint32_t first, uint32_t n, rmq_scrub_res* res);
/* Fault injection (tests): XORs the byte at ring_off of replica slot `replica`'s ring of pidx
   (addressed as rmq_read_segment addresses it) with the low 8 bits of xor_mask, as a memory
   corruption would. RMQ_EINVAL for a slot this engine does not hold, ring_off >= the ring's bytes
   or a zero mask. Drains first (collective with a transport, like rmq_sync). */
int rmq_fault_flip_ring(rmq_engine* e, uint32_t replica, uint32_t pidx, uint64_t ring_off, uint32_t xor_mask);

/* ---- repair (added after ABI 11 without a bump: one struct, one flag and one function, and no
   existing struct, value or behaviour moves, so every ABI 11 caller still links and runs) ---- */
#define RMQ_REPAIR_DRY_RUN 1u   /* find and count, write nothing */
typedef struct rmq_repair_res {
  uint64_t segments_repaired;    /* (local slot, segment) pairs rewritten from a clean local slot */
  uint64_t bytes_repaired;       /* their segment bytes (end - pos of each) */
  uint64_t segments_unrepaired;  /* failing pairs with no passing local slot for that segment: left as they were */
  uint64_t bad_offset;           /* what remains AFTER the call, as rmq_scrub_res reports it */
  uint32_t bad_replica;
  uint32_t bad_kind;
  uint32_t replicas;
  int32_t status;                /* RMQ_OK, or RMQ_ECORRUPT if something remains */
} rmq_repair_res;                /* 48 bytes */
/* Scrub, then repair, then scrub again (FORMAT.md §10 "Repair"): audits partitions [first, first + n)
   as the scrub does, and overwrites the bytes of every (local slot, segment) pair that fails with
   those of the lowest local slot on which the same segment passes. Nothing else is written: bytes
   outside retained segments, passing pairs, index entries, partition state, consumer offsets and
   the position cache stay. A failing pair with no passing local slot (a single local slot, damage
   on every slot, a damaged index entry or partition state) is counted in segments_unrepaired and
   left alone. The range is then audited again: bad_offset, bad_replica, bad_kind, replicas and
   status are the scrub's row of the state the call leaves. With RMQ_REPAIR_DRY_RUN the counters
   are those the real call would return, the other fields describe the present state and no ring
   byte changes. res (host, [n], nullable). Returns RMQ_OK if every partition of the range is clean
   afterwards, RMQ_ECORRUPT if any is not, RMQ_ENOPART if the range leaves [0, P), RMQ_EINVAL for an
   unknown flag bit. Drains first: with a transport attached the call is collective, and each rank
   repairs only the slots it holds. */
int rmq_repair(rmq_engine* e, uint32_t first, uint32_t n, uint32_t flags, rmq_repair_res* res);

/* ---- index rebuild (added after ABI 11 without a bump, as rmq_repair was: one struct, two flags
   and two functions, nothing existing moves) ---- */
#define RMQ_REINDEX_DRY_RUN 1u  /* walk and count, write nothing */
#define RMQ_REINDEX_ALL     2u  /* trust no stored entry: one walk per partition from the log start */
typedef struct rmq_reindex_res {
  uint64_t entries_live;       /* live entries of the partition, hi - lo + 1 (0 if none) */
  uint64_t entries_rewritten;  /* live entries whose stored value the call changed (dry run: would change) */
  uint64_t gaps_unresolved;    /* gaps whose walk did not complete: their entries are left as they were */
  uint64_t bad_offset;         /* what remains AFTER the call, as rmq_scrub_res reports it */
  uint32_t bad_replica;
  uint32_t bad_kind;
  uint32_t replicas;
  int32_t status;              /* RMQ_OK, or RMQ_ECORRUPT if something remains */
} rmq_reindex_res;             /* 48 bytes */
/* Scrub, then rebuild damaged sparse-index entries from the log, then scrub again (FORMAT.md §10
   "Index rebuild"). The index is one per partition, so a damaged entry fails its two adjoining
   segments on every local slot alike and neither repair has a donor for it; the records that define
   it are intact on the slots. The first pass is rmq_repair's. A segment that passes on no local slot
   is bad, a maximal run of bad segments is a gap, and one walk per gap starts at the gap's start
   boundary (the log start, or the stored entry that ends the passing segment before it) and
   accepts each record that passes the scrub's checks on some local slot, lowest slot first, so a
   record damaged on one slot does not stop it. Entry m is {offset, pos} of the first record start
   at logical position >= m * interval, the log end counting as one. A gap is resolved when its
   walk reaches the stored entry that ends it with exactly that value (the log end, for a gap that
   ends the log); only then are its live entries that differ from the rebuilt ones written, and the
   partition's position-cache rows emptied. An unresolved gap (a record that passes on no slot or
   runs past the span, another value at the gap's end, a partition state no log can have) is counted
   in gaps_unresolved and nothing of it is written. With RMQ_REINDEX_ALL there is one walk per
   partition with a local slot, from the log start to the log end, trusting no stored entry: the
   only mode that corrects an entry the scrub passes because it names a true record start that is
   not the first one at or after its multiple; it is serial per partition. Ring bytes, partition
   state, consumer offsets and index slots outside the live range are never written. The range is
   then audited again: bad_offset, bad_replica, bad_kind, replicas and status are the scrub's row
   of the state the call leaves. With RMQ_REINDEX_DRY_RUN the counters are those the real call
   would return, the other fields describe the present state and no byte changes. Call order for a
   damaged replica: rmq_reindex, then rmq_repair, then rmq_repair_remote. res (host, [n], nullable).
   Returns RMQ_OK if every partition of the range is clean afterwards, RMQ_ECORRUPT if any is not,
   RMQ_ENOPART if the range leaves [0, P), RMQ_EINVAL for an unknown flag bit. Drains first: with a
   transport attached the call is collective, and each rank rebuilds its own index. */
int rmq_reindex(rmq_engine* e, uint32_t first, uint32_t n, uint32_t flags, rmq_reindex_res* res);
/* Fault injection (tests): XORs xor_mask into word `word` (0 offset, 1 pos) of index slot
   m mod icap of pidx, as a memory corruption would. RMQ_ENOPART for a bad pidx, RMQ_EINVAL for
   word > 1 or a zero mask. Drains first (collective with a transport, like rmq_sync). */
int rmq_fault_flip_index(rmq_engine* e, uint32_t pidx, uint64_t m, uint32_t word, uint64_t xor_mask);

/* ---- remote repair (added after ABI 11 without a bump, as rmq_repair was: one struct and two
   functions, nothing existing moves) ---- */
typedef struct rmq_repair_remote_res {
  uint64_t segments_repaired;    /* as rmq_repair_res: rewritten from a clean local slot */
  uint64_t bytes_repaired;
  uint64_t segments_fetched;     /* failing pairs rewritten with bytes a peer served */
  uint64_t bytes_fetched;        /* their segment bytes (end - pos of each) */
  uint64_t segments_unrepaired;  /* failing pairs left as they were after every round */
  uint64_t bad_offset;           /* what remains AFTER the call, as rmq_scrub_res reports it */
  uint32_t bad_replica;
  uint32_t bad_kind;
  uint32_t replicas;
  int32_t status;                /* RMQ_OK, or RMQ_ECORRUPT if something remains */
} rmq_repair_remote_res;         /* 64 bytes */
/* rmq_repair, then the pairs it had to leave are fetched from the ranks that hold the partition's
   other replica slots (FORMAT.md §10 "Remote repair"). Pass 0 is rmq_repair's audit and local copy.
   A pair still failing whose segment has bounds and whose records are all at or below this
   replica's commit is then asked of one candidate rank per round, RF - 1 rounds: the leader's rank
   first, then the other slots' ranks by ascending slot. The donor checks every request word against
   its own state, walks the span in its own ring under the rules of the verified fetch and sends
   only a span that passes; the requester walks the span again where it arrived and only then copies
   it into the failing slot's ring, so no unverified byte reaches a ring. What is never written is
   what rmq_repair never writes; an uncommitted tail is never fetched. The range is then audited
   again and the rows report what remains. flags: 0 or RMQ_REPAIR_DRY_RUN (the same exchanges,
   directory-only responses, the counters of the real call, no ring byte changes anywhere); any
   other bit is RMQ_EINVAL. res (host, [n], nullable); served (nullable, [2]) gets {segments, bytes}
   this engine sent as a donor. Returns as rmq_repair does. Without a transport the call does
   exactly what rmq_repair does (segments_fetched = 0, served = {0, 0}). With a transport it is
   collective: every rank makes it at the same point of its call sequence with the same flags;
   [first, first + n) is local to each rank, may differ between ranks and only selects which of this
   rank's partitions are repaired: every rank serves every peer's requests whatever its own range,
   and a rank with n = 0 still takes part as a donor. Per round and destination at most 65,536 pairs
   and RMQ_REPAIR_PEER_BYTES (environment, read at rmq_create; default 64 MiB, a capacity and not a
   tuned number) of segment bytes are asked for; the rest waits for a later round or call. */
int rmq_repair_remote(rmq_engine* e, uint32_t first, uint32_t n, uint32_t flags, rmq_repair_remote_res* res,
                      uint64_t* served);
/* Fault injection (tests): the next remote-repair response this engine sends to rank dst has the
   byte at `at` of its data section XORed with 0x5A (at < 0: counted back from the end of the data
   section); a response without that byte is sent as it is and uses the flip up. Independent of
   rmq_fault_corrupt, whose pending flip belongs to the next replication round. Not collective. */
int rmq_fault_corrupt_repair(rmq_engine* e, uint32_t dst, int64_t at);

/* ---- restore (added after ABI 11 without a bump, as the repairs were: two structs, one flag and
   one function, nothing existing moves) ---- */
#define RMQ_RESTORE_DRY_RUN 1u          /* verify and report, write nothing */
typedef struct rmq_restore_item {        /* 64 bytes */
  uint32_t pidx;
  uint32_t flags;        /* 0 */
  uint64_t first_offset; /* header offset of the run's first record = the new log_start_offset */
  uint64_t first_pos;    /* logical position it takes = the new log_start_pos; multiple of 16 */
  uint64_t count;        /* records in the run */
  uint64_t bytes;        /* run bytes; the run is buf[buf_pos, buf_pos + bytes) */
  uint64_t buf_pos;      /* multiple of 16 */
  uint64_t table_start;  /* rec_pos[table_start + k], k in [0, count]: record k's byte position inside
                            the run, then the run's end (== bytes): what rmq_scan_records /
                            rmq_tier_append write as pos_out */
  uint64_t commit;       /* the replica's commit after the restore, in [first_offset, first_offset + count] */
} rmq_restore_item;
typedef struct rmq_restore_res {         /* 32 bytes */
  uint64_t records;      /* records installed (dry run: that would be) */
  uint64_t bytes;
  uint64_t bad_offset;   /* lowest expected offset of a failing record; RMQ_OFFSET_NONE if none */
  uint32_t bad_kind;     /* RMQ_SCRUB_BAD_CRC / RMQ_SCRUB_BAD_CHAIN */
  int32_t status;        /* RMQ_OK, RMQ_ECORRUPT, RMQ_EINVAL, RMQ_ENOSPC, RMQ_ENOPART */
} rmq_restore_res;
/* Loads replica logs from FORMAT.md §1 record images (segment files of a durable tier) on the device
   (FORMAT.md §11 "Restore"). Item i restarts the pristine partition items[i].pidx (log start and end
   offsets and positions all 0) as the log [first_offset, first_offset + count) at logical positions
   [first_pos, first_pos + bytes), from the run buf[buf_pos, buf_pos + bytes) and its record
   positions rec_pos[table_start .. table_start + count]. items, rec_pos (rec_words words) and res
   ([n], nullable) are host arrays; buf (buf_bytes bytes, 16-byte aligned) is RMQ_MEM_HOST or
   RMQ_MEM_DEVICE; a host buffer and the table go to device scratch the engine keeps (RMQ_ENOMEM,
   nothing changed, if it cannot be allocated). A row that fails the host checks (RMQ_ENOPART,
   RMQ_ENOSPC: bytes over the ring, RMQ_EINVAL: alignment, ranges, counts, commit, flags, a partition
   that is not pristine, named twice or without a local slot) is skipped and the others proceed. On
   the device every record is verified first, a lane per record: the table tiles the run, header
   offsets run first_offset + k, each record's size is the distance to the next table word, CRC32C
   and zero padding; no table or length word is an address before these hold. A partition with any
   failing record gets RMQ_ECORRUPT with the lowest failing expected offset and its kind and stays
   pristine in every respect. A partition that passes is installed: the run into every local replica
   slot's ring at pos mod S_p, the sparse index entries of §5, log start (first_offset, first_pos),
   log end, commit = high_watermark = leader_commit = item.commit, match of the local slots = the log
   end and of the others 0, both state sets, its position-cache entries emptied. Terms, votes,
   leadership and consumer offsets are not touched (rmq_become_leader, rmq_set_vote,
   rmq_commit_consumer_offset restore them). flags: 0 or RMQ_RESTORE_DRY_RUN (the rows of the real
   call, nothing written); any other bit is RMQ_EINVAL, and so are a null engine, null items with
   n != 0, an unknown mem and an attached transport (a restarted rank restores before it attaches).
   Returns RMQ_OK if every row is, else the status of the lowest-index row that is not. Drains first. */
int rmq_restore(rmq_engine* e, uint32_t n, const rmq_restore_item* items, uint32_t mem,
                const uint8_t* buf, uint64_t buf_bytes, const uint64_t* rec_pos, uint64_t rec_words,
                uint32_t flags, rmq_restore_res* res);

/* ---- host utilities ---- */
/* FORMAT.md §1 records laid back to back in host memory (segment files of a durable tier, fetch
   output): walks them from buf[0], expecting header offsets first, first + 1, ..., and stops at the
   first record that is out of sequence or cut short, or (flags & RMQ_SCAN_CHECK) whose CRC32C or
   zero padding is wrong, or after max_records. *count / *bytes = the whole records before that;
   pos_out (nullable, max_records + 1 slots) gets each one's byte position and then the end. Needs no
   engine (or GPU). */
#define RMQ_SCAN_CHECK 1u
int rmq_scan_records(const uint8_t* buf, uint64_t len, uint64_t first, uint64_t max_records, uint32_t flags,
                     uint64_t* pos_out, uint64_t* count, uint64_t* bytes);
/* Durable-tier spill (ripplemq_amd/tier.py; jraft's per-group log, PartitionRaftServer.java:53,88-90):
   run i = buf[buf_pos[i], buf_pos[i] + bytes[i]), count[i] back-to-back FORMAT.md §1 records with
   header offsets first[i], first[i] + 1, ... (as one rmq_fetch returns a partition's slice), is
   appended to the open file descriptor fd[i]; pos_out gets, run after run, each record's position
   inside its run and then the run's end (count[i] + 1 words per run). Runs are checked first
   (RMQ_EINVAL, nothing written); the writes go over `threads` threads (0: up to 8); fsync_each != 0
   fsyncs every file. RMQ_EDEVICE on an I/O error (errno set). Needs no engine (or GPU). */
int rmq_tier_append(uint32_t n, const int32_t* fd, const uint64_t* first, const uint64_t* count,
                    const uint64_t* buf_pos, const uint64_t* bytes, const uint8_t* buf, uint64_t* pos_out,
                    uint32_t threads, int fsync_each);

/* ---- device buffers and timing (bench / tests keep inputs resident in HBM) ---- */
int rmq_device_alloc(rmq_engine* e, uint64_t bytes, void** out);
int rmq_device_free(rmq_engine* e, void* p);
int rmq_memcpy(rmq_engine* e, void* dst, const void* src, uint64_t bytes, int kind /*0 h2d,1 d2h,2 d2d*/);
/* Page-locked host memory for RMQ_MEM_PINNED batches (reference side: the JNI layer's direct
   ByteBuffers): allocate, or register / unregister existing pages. */
int rmq_host_alloc(rmq_engine* e, uint64_t bytes, void** out);
int rmq_host_free(rmq_engine* e, void* p);  /* e may be NULL (buffers outliving the engine) */
int rmq_host_register(rmq_engine* e, void* p, uint64_t bytes);
int rmq_host_unregister(rmq_engine* e, void* p);
/* Kernel timing with HIP events on the engine's stream (enable != 0 turns it on and resets it).
   kernels 0 and 1: the pipeline launches from the first one after enable up to the next drain
   (sync, control call, read-back) timed as ONE region (no events between launches): total_ms =
   region time; launches = pipeline launches in it (kernel 0) or batches they applied (kernel 1).
   kernel 3: rmq_fetch, the summed dispatch-recorded spans of its kernels; 4: rmq_fetch, an event
   before its first kernel to one after its last (the request copy before and the result copy after
   outside), launches = kernel executions. enable = k >= 2 also runs every fetch's kernels k times
   back to back (idempotent: the same results), so kernel 4 / launches is a kernel time that no
   copy or host gap inflates and a rocprofv3 trace shows the kernels back to back; a fetch with an
   RMQ_FETCH_COMMIT or RMQ_FETCH_VERIFY request runs once (each run would commit; the verify
   rewrites the rows). 2: rmq_scrub, an event before its first kernel (the plan) to one after its last
   (the verify), launches = calls. 5: rmq_repair, likewise from before its first kernel to after its
   last, launches = calls. 6: rmq_repair_remote, from before its first plan to after its last kernel
   (the exchanges and the host's waits between them included), launches = calls. 7: rmq_restore, an
   event before its first kernel to one after its last (the staging copies before them outside),
   launches = calls. 8: rmq_reindex, an event before its first plan to one after its last kernel,
   launches = calls. 9: the record-table kernels of rmq_fetch_table, an event before the first to one
   after the last, launches = calls (such a fetch runs once, without dispatch spans, as a budgeted
   one; its table kernels lie inside its region 4 too). 10: rmq_lag, an event before its kernel to one
   after it, launches = calls. 11: rmq_unpack, an event before its first kernel to one after its
   last, launches = calls. */
int rmq_profile_enable(rmq_engine* e, int enable);
int rmq_profile_query(rmq_engine* e, int kernel, uint64_t* launches, double* total_ms);
/* Device name / CU count for reports. */
int rmq_device_info(rmq_engine* e, char* name, uint32_t name_cap, uint32_t* cu_count);

#ifdef __cplusplus
}
#endif
#endif /* RIPPLEMQ_ENGINE_H */
