#!/usr/bin/env python3
"""Load/wait skeleton of a disassembled kernel: from an `llvm-objdump -d` listing of pipeline.hip
(compiled with --cuda-device-only --no-gpu-bundle-output), print only the memory loads, the waits,
the barriers, the branches and the first stores of a line range, with the encoding comments cut.

  tools/s3_skeleton.py listing.s FIRST LAST      # lines FIRST..LAST of the listing (1-based)
  tools/s3_skeleton.py listing.s --find-span     # line numbers of the span loads (buffer_load ... nt)
"""
import re
import sys

KEEP = re.compile(
    r"^\s*(global_load|buffer_load|flat_load|s_load|s_buffer_load|s_waitcnt|s_barrier|s_cbranch|s_branch|"
    r"global_store|buffer_store|flat_store|ds_write|ds_read|s_endpgm|s_setprio|s_memrealtime)")


def main() -> None:
    lines = open(sys.argv[1]).read().splitlines()
    if sys.argv[2] == "--find-span":
        for n, ln in enumerate(lines, 1):
            if "buffer_load_dwordx4" in ln and " nt" in ln:
                print(n, ln.split("//")[0].strip())
        return
    first, last = int(sys.argv[2]), int(sys.argv[3])
    run_kind, run_n = None, 0

    def flush() -> None:
        nonlocal run_kind, run_n
        if run_kind and run_n:
            print(f"        ... {run_n} x {run_kind}")
        run_kind, run_n = None, 0

    for n in range(first, last + 1):
        ln = lines[n - 1]
        if re.match(r"^[0-9a-f]+ <", ln):
            flush()
            print(f"{n:6d}  {ln}")
            continue
        if not KEEP.match(ln):
            continue
        text = ln.split("//")[0].strip()
        op = text.split()[0]
        if op in ("ds_write_b32", "ds_read_b32", "ds_read2_b32", "ds_write2_b32", "ds_read_b128", "ds_write_b128",
                  "ds_read2_b64", "ds_write_b64", "ds_read_b64", "ds_read2st64_b32"):
            if run_kind != op:
                flush()
                run_kind = op
            run_n += 1
            continue
        flush()
        print(f"{n:6d}  {text}")
    flush()


if __name__ == "__main__":
    main()
