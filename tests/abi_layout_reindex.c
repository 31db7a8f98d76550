/* Prints sizeof/offsetof of rmq_reindex_res and the constants next to it (compiled by
   tests/test_reindex_abi.py with gcc). */
#include <stddef.h>
#include <stdio.h>
#include "../include/ripplemq_engine.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("rmq_reindex_res %zu\n", sizeof(rmq_reindex_res));
  F(rmq_reindex_res, entries_live); F(rmq_reindex_res, entries_rewritten); F(rmq_reindex_res, gaps_unresolved);
  F(rmq_reindex_res, bad_offset); F(rmq_reindex_res, bad_replica); F(rmq_reindex_res, bad_kind);
  F(rmq_reindex_res, replicas); F(rmq_reindex_res, status);
  printf("RMQ_ABI_VERSION %u\n", RMQ_ABI_VERSION);
  printf("RMQ_REINDEX_DRY_RUN %u\n", RMQ_REINDEX_DRY_RUN);
  printf("RMQ_REINDEX_ALL %u\n", RMQ_REINDEX_ALL);
  return 0;
}
