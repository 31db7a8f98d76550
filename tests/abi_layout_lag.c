/* Prints sizeof/offsetof of rmq_lag_res and the sizes and constants the addition must leave alone
   (compiled by tests/test_lag_abi.py with gcc -Wall -Werror). */
#include <stddef.h>
#include <stdio.h>
#include "../include/ripplemq_engine.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("rmq_lag_res %zu\n", sizeof(rmq_lag_res));
  F(rmq_lag_res, start_offset); F(rmq_lag_res, records); F(rmq_lag_res, bytes); F(rmq_lag_res, evicted);
  F(rmq_lag_res, start_pos); F(rmq_lag_res, end_pos); F(rmq_lag_res, headroom); F(rmq_lag_res, status);
  F(rmq_lag_res, reserved);
  printf("rmq_fetch_req %zu\n", sizeof(rmq_fetch_req));
  printf("rmq_fetch_res %zu\n", sizeof(rmq_fetch_res));
  printf("RMQ_ABI_VERSION %u\n", RMQ_ABI_VERSION);
  return 0;
}
/* the declaration itself: a second one compiles only if it matches the header's */
typedef int lag_fn(rmq_engine*, const rmq_fetch_req*, const uint64_t*, uint32_t, uint32_t, rmq_lag_res*);
extern lag_fn rmq_lag;
