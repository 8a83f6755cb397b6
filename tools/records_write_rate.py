#!/usr/bin/env python3
"""The rate of records_write_kernel (mdbg_minimizers_to_record_bytes) on one resident scan output, both forms, from the library's own
"records_write" timer (device events around the launch):

    python tools/records_write_rate.py --reads 1000000 --calls 10

One process, one JSON line; run it several times for the spread.  Bytes READ are counted from the arrays the kernel walks (offsets,
values and, for INIT, positions, directions, qualities, lengths and mean qualities -- 4 bytes a read also when the set carries one value
for all of them), bytes WRITTEN are the record bytes; GB/s is their sum over
the kernel time.  The first call of each form is a warm-up and is not timed."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    from metamdbg_amd import capi, synth
    ctx = capi.Context(0)
    reads = ctx.reads_synthetic(synth.hifi_spec(a.reads, seed=42, read_len=a.read_len, coverage=50.0))
    mins = ctx.scan(reads, K=15, density=0.005, hpc=True)
    reads.free()
    n, t = mins.info()["n_reads"], mins.info()["n_minimizers"]
    mins.device_ptrs()                      # the fresh output brought into read order once, outside the timer
    res = {"reads": n, "minimizers": t, "calls": a.calls}
    for name, form in (("plain", capi.RECORDS_PLAIN), ("init", capi.RECORDS_INIT)):
        ctx.minimizers_to_record_bytes(mins, form).free()
        ctx.synchronize()
        ctx.timing(True)
        ctx.timing_reset()
        n_bytes = 0
        for _ in range(a.calls):
            b = ctx.minimizers_to_record_bytes(mins, form)
            n_bytes = b.n
            ctx.synchronize()
            b.free()
        ms, launches = ctx.timing_get("records_write")
        ctx.timing(False)
        assert launches == a.calls
        read = 8 * (n + 1) + 4 * t + (6 * t + 8 * n if form == capi.RECORDS_INIT else 0)
        per = ms / launches
        res[name] = {"ms_per_launch": per, "bytes_written": n_bytes, "bytes_read": read, "gb_per_s_read_plus_written": (read + n_bytes) / per / 1e6}
    print(json.dumps(res))
    mins.free()
    ctx.close()


if __name__ == "__main__":
    main()
