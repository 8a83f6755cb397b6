#!/usr/bin/env python3
"""The rates of mdbg_kminmer_spans's two steps on one resident batch, beside the scan of the same batch, from the library's own timers
(device events around the launches): "scan", "spans_map" (the tile counts with the per-read sums, then the selects: two groups of launches a
call) and "spans_windows".

    python tools/spans_rate.py --reads 1000000 --calls 5

Synthetic HiFi reads (mdbg_reads_synthetic), homopolymer compression, l 15, density 0.005, k 4.  Each kernel's rate is taken against its
ALGORITHMIC bytes:
    map      0.25 B a base read + 8 B a minimizer read (offset share and position) + 8 B a minimizer written (S and E)
    windows  4 B a minimizer read + 33 B a window written (identity 16, reversed 1, four fields 16)
What the map moves beyond that -- two bytes a word of offsets written and partly read again, the words around a query read a second
time -- is in its time, not in its bytes.  The first call is a warm-up and is not timed; run the tool several times for the spread."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--k", type=int, default=4)
    a = ap.parse_args()
    from metamdbg_amd import capi, synth
    ctx = capi.Context(0)
    reads = ctx.reads_synthetic(synth.hifi_spec(a.reads, seed=42, read_len=a.read_len, coverage=50.0))
    bases = reads.info()["n_bases"]
    scan = lambda: ctx.scan(reads, K=15, density=0.005, hpc=True, apply_read_filters=False)
    scan().free()                            # warm-up
    ctx.synchronize()
    ctx.timing(True)
    ctx.timing_reset()
    for _ in range(a.calls):
        m = scan()
        ctx.synchronize()
        m.free()
    scan_ms, scan_n = ctx.timing_get("scan")
    ctx.timing(False)
    mins = scan()
    mins.device_ptrs()                       # the fresh output brought into read order once, outside the timers
    n_min = mins.info()["n_minimizers"]
    ctx.kminmer_spans(reads, mins, K=15, hpc=True, k=a.k).free()
    ctx.synchronize()
    ctx.timing(True)
    ctx.timing_reset()
    n_win = 0
    for _ in range(a.calls):
        sp = ctx.kminmer_spans(reads, mins, K=15, hpc=True, k=a.k)
        n_win = sp.info()["n_windows"]
        sp.free()
    map_ms, map_n = ctx.timing_get("spans_map")
    win_ms, win_n = ctx.timing_get("spans_windows")
    ctx.timing(False)
    assert map_n == 2 * a.calls and win_n == a.calls and scan_n >= a.calls
    scan_per, map_per, win_per = scan_ms / a.calls, map_ms / a.calls, win_ms / a.calls
    map_bytes = 0.25 * bases + 16 * n_min
    win_bytes = 4 * n_min + 33 * n_win
    print(f"reads {a.reads} x {a.read_len} bases = {bases} bases, {n_min} minimizers, k {a.k}: {n_win} windows; {a.calls} timed calls")
    print(f"scan           {scan_per:9.3f} ms a call   {bases / scan_per / 1e6:8.2f} Gbp/s   ({scan_n} launches)")
    print(f"spans_map      {map_per:9.3f} ms a call   {bases / map_per / 1e6:8.2f} Gbp/s   {map_bytes / map_per / 1e6:8.1f} GB/s of {map_bytes / 1e6:.1f} MB algorithmic")
    print(f"spans_windows  {win_per:9.3f} ms a call   {n_win / win_per / 1e6:8.2f} G windows/s   {win_bytes / win_per / 1e6:8.1f} GB/s of {win_bytes / 1e6:.1f} MB algorithmic")
    print(f"map / scan     {map_per / scan_per:9.3f}")
    mins.free()
    reads.free()
    ctx.close()


if __name__ == "__main__":
    main()
