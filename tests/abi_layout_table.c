/* Prints what rmq_fetch_table's declaration rests on, and checks the two functions' prototypes
   against the argument list FORMAT.md gives (compiled by tests/test_fetch_table_abi.py with gcc, not
   linked against the engine: the assignments stand inside sizeof, type-checked and never evaluated). */
#include <stdio.h>
#include "../include/ripplemq_engine.h"
typedef int (*table_fn)(rmq_engine*, const rmq_fetch_req*, const uint64_t*, const uint32_t*, uint32_t, uint32_t,
                        uint8_t*, uint64_t, rmq_fetch_res*, uint64_t*, uint64_t*, uint64_t, uint64_t*);
int main(int argc, char** argv) {
  table_fn f = 0;
  (void)argc, (void)argv;
  printf("declared %u\n", (unsigned)(sizeof(f = rmq_fetch_table) == sizeof(f = rmq_fetch_table_async)));
  printf("RMQ_ABI_VERSION %u\n", RMQ_ABI_VERSION);
  printf("sizeof_rmq_fetch_res %u\n", (unsigned)sizeof(rmq_fetch_res));
  printf("sizeof_rmq_fetch_req %u\n", (unsigned)sizeof(rmq_fetch_req));
  printf("sizeof_rmq_restore_item %u\n", (unsigned)sizeof(rmq_restore_item));
  printf("RMQ_MEM_HOST %u\n", (unsigned)RMQ_MEM_HOST);
  printf("RMQ_MEM_DEVICE %u\n", (unsigned)RMQ_MEM_DEVICE);
  printf("RMQ_FETCH_FILL %u\n", RMQ_FETCH_FILL);
  printf("RMQ_ENOSPC %d\n", (int)RMQ_ENOSPC);
  printf("RMQ_EINVAL %d\n", (int)RMQ_EINVAL);
  return 0;
}
