/* Prints the `mem` bits of a fetch call and the codes a filling fetch answers (compiled by
   tests/test_fetch_fill_abi.py with gcc). */
#include <stdio.h>
#include "../include/ripplemq_engine.h"
int main(void) {
  printf("RMQ_FETCH_FILL %u\n", RMQ_FETCH_FILL);
  printf("RMQ_FETCH_PINNED_ROWS %u\n", RMQ_FETCH_PINNED_ROWS);
  printf("RMQ_FETCH_DEVICE_ROWS %u\n", RMQ_FETCH_DEVICE_ROWS);
  printf("RMQ_MEM_HOST %u\n", (unsigned)RMQ_MEM_HOST);
  printf("RMQ_MEM_DEVICE %u\n", (unsigned)RMQ_MEM_DEVICE);
  printf("RMQ_MEM_PINNED %u\n", (unsigned)RMQ_MEM_PINNED);
  printf("RMQ_PENDING %d\n", (int)RMQ_PENDING);
  printf("RMQ_ENOSPC %d\n", (int)RMQ_ENOSPC);
  printf("RMQ_ABI_VERSION %u\n", RMQ_ABI_VERSION);
  printf("sizeof_rmq_fetch_res %u\n", (unsigned)sizeof(rmq_fetch_res));
  return 0;
}
