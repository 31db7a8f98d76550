/* Prints sizeof/offsetof of rmq_restore_item and rmq_restore_res and the constants next to them
   (compiled by tests/test_restore_abi.py with gcc). */
#include <stddef.h>
#include <stdio.h>
#include "../include/ripplemq_engine.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("rmq_restore_item %zu\n", sizeof(rmq_restore_item));
  printf("rmq_restore_res %zu\n", sizeof(rmq_restore_res));
  F(rmq_restore_item, pidx); F(rmq_restore_item, flags); F(rmq_restore_item, first_offset);
  F(rmq_restore_item, first_pos); F(rmq_restore_item, count); F(rmq_restore_item, bytes);
  F(rmq_restore_item, buf_pos); F(rmq_restore_item, table_start); F(rmq_restore_item, commit);
  F(rmq_restore_res, records); F(rmq_restore_res, bytes); F(rmq_restore_res, bad_offset);
  F(rmq_restore_res, bad_kind); F(rmq_restore_res, status);
  printf("RMQ_ABI_VERSION %u\n", RMQ_ABI_VERSION);
  printf("RMQ_RESTORE_DRY_RUN %u\n", RMQ_RESTORE_DRY_RUN);
  return 0;
}
