/* Prints sizeof/offsetof of rmq_scrub_res and the ABI 11 constants (compiled by
   tests/test_scrub_abi.py with gcc). */
#include <stddef.h>
#include <stdio.h>
#include "../include/ripplemq_engine.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("rmq_scrub_res %zu\n", sizeof(rmq_scrub_res));
  F(rmq_scrub_res, records_ok); F(rmq_scrub_res, bytes_ok); F(rmq_scrub_res, bad_offset);
  F(rmq_scrub_res, bad_replica); F(rmq_scrub_res, bad_kind); F(rmq_scrub_res, replicas);
  F(rmq_scrub_res, status);
  printf("RMQ_ABI_VERSION %u\n", RMQ_ABI_VERSION);
  printf("RMQ_ECORRUPT %d\n", (int)RMQ_ECORRUPT);
  printf("RMQ_FETCH_VERIFY %u\n", RMQ_FETCH_VERIFY);
  printf("RMQ_SCRUB_BAD_CRC %u\n", RMQ_SCRUB_BAD_CRC);
  printf("RMQ_SCRUB_BAD_CHAIN %u\n", RMQ_SCRUB_BAD_CHAIN);
  return 0;
}
