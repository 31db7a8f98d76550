/* Prints sizeof/offsetof of rmq_repair_remote_res and the constants next to it (compiled by
   tests/test_repair_remote_abi.py with gcc). */
#include <stddef.h>
#include <stdio.h>
#include "../include/ripplemq_engine.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("rmq_repair_remote_res %zu\n", sizeof(rmq_repair_remote_res));
  F(rmq_repair_remote_res, segments_repaired); F(rmq_repair_remote_res, bytes_repaired);
  F(rmq_repair_remote_res, segments_fetched); F(rmq_repair_remote_res, bytes_fetched);
  F(rmq_repair_remote_res, segments_unrepaired); F(rmq_repair_remote_res, bad_offset);
  F(rmq_repair_remote_res, bad_replica); F(rmq_repair_remote_res, bad_kind);
  F(rmq_repair_remote_res, replicas); F(rmq_repair_remote_res, status);
  printf("RMQ_ABI_VERSION %u\n", RMQ_ABI_VERSION);
  printf("RMQ_REPAIR_DRY_RUN %u\n", RMQ_REPAIR_DRY_RUN);
  return 0;
}
