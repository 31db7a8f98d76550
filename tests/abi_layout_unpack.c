/* Prints sizeof/offsetof of rmq_unpack_args and rmq_unpack_res and the sizes and constants the
   addition must leave alone (compiled by tests/test_unpack_abi.py with gcc -Wall -Werror). */
#include <stddef.h>
#include <stdio.h>
#include "../include/ripplemq_engine.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("rmq_unpack_args %zu\n", sizeof(rmq_unpack_args));
  F(rmq_unpack_args, buf); F(rmq_unpack_args, buf_bytes); F(rmq_unpack_args, rows); F(rmq_unpack_args, rec_row);
  F(rmq_unpack_args, rec_pos); F(rmq_unpack_args, rec_words); F(rmq_unpack_args, row_tag); F(rmq_unpack_args, rec_first);
  F(rmq_unpack_args, offset); F(rmq_unpack_args, len); F(rmq_unpack_args, payload_off); F(rmq_unpack_args, tag);
  F(rmq_unpack_args, rec_cap); F(rmq_unpack_args, payload); F(rmq_unpack_args, payload_cap); F(rmq_unpack_args, n);
  F(rmq_unpack_args, stride); F(rmq_unpack_args, mem); F(rmq_unpack_args, flags);
  printf("rmq_unpack_res %zu\n", sizeof(rmq_unpack_res));
  F(rmq_unpack_res, records); F(rmq_unpack_res, payload_bytes); F(rmq_unpack_res, mismatched); F(rmq_unpack_res, truncated);
  F(rmq_unpack_res, bad_row); F(rmq_unpack_res, status); F(rmq_unpack_res, reserved);
  printf("rmq_fetch_req %zu\n", sizeof(rmq_fetch_req));
  printf("rmq_fetch_res %zu\n", sizeof(rmq_fetch_res));
  printf("rmq_lag_res %zu\n", sizeof(rmq_lag_res));
  printf("rmq_batch %zu\n", sizeof(rmq_batch));
  printf("rmq_restore_item %zu\n", sizeof(rmq_restore_item));
  printf("RMQ_ABI_VERSION %u\n", RMQ_ABI_VERSION);
  return 0;
}
/* the declaration itself: a second one compiles only if it matches the header's */
typedef int unpack_fn(rmq_engine*, const rmq_unpack_args*, rmq_unpack_res*);
extern unpack_fn rmq_unpack;
