#!/usr/bin/env python3
"""The rates of mdbg_map_verify on one resident batch, from the library's own timers (device events around the launches): "verify_join" (the
lookup's keys, the rows' reads, count and fill), "radix_sort" (the lookup's one sort of the set's minimizers), "verify_chains", "verify_rows"
-- beside a device-to-device copy of as many bytes as each step's algorithmic bytes, timed in the same process: the yardstick, which reads
and writes that many bytes and does nothing else.

    python tools/verify_rate.py --genome 100000 --runs 3

Input: the synthetic genome of tools/map_rate.py in minimizer space (random u32 minimizers 20 - 60 apart), reads of about 250 minimizers at
20-fold coverage, half of them on the reverse strand (directions flipped), 2 % of the minimizers changed, uploaded with positions, directions
and lengths.  The selection is the mapper's own: index, anchors, chains, mdbg_map_select at coverage 20; then mdbg_map_verify at band 62,
overhang 1000, overlap 1000, identity 0.96, size 15.
ALGORITHMIC bytes.  join: 12 B a minimizer of the set (the lookup written) + per row the two reads' minimizers (4 B each, read twice: count
and fill) and the neighbour's lookup (8 B a minimizer, twice) + 17 B an anchor written.  chains: 17 B an anchor read + 64 B a row written.
rows: 64 B a row read + 4 B its flag + 12 B the scan + 5 B a kept row.  The first call is a warm-up and is not timed."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_reads(genome: int, read_len: int, coverage: float, seed: int):
    rng = np.random.default_rng(seed)
    g = rng.integers(1, 1 << 32, genome, dtype=np.uint64).astype(np.uint32)
    gdir = rng.integers(0, 2, genome).astype(np.uint8)
    gpos = np.cumsum(rng.integers(20, 60, genome))
    n_reads = int(coverage * genome / read_len)
    start = rng.integers(0, genome - read_len, n_reads)
    at = start[:, None] + np.arange(read_len)[None, :]
    mins, dirs, pos = g[at], gdir[at], gpos[at] - gpos[start][:, None] + rng.integers(0, 200, n_reads)[:, None]
    changed = rng.random(mins.shape) < 0.02
    mins[changed] = rng.integers(1, 1 << 32, int(changed.sum()), dtype=np.uint64).astype(np.uint32)
    length = pos[:, -1] + 100
    rev = rng.random(n_reads) < 0.5
    mins[rev] = mins[rev, ::-1]
    dirs[rev] = 1 - dirs[rev, ::-1]
    pos[rev] = length[rev, None] - 1 - pos[rev, ::-1]
    return mins.reshape(-1), np.arange(n_reads + 1, dtype=np.uint64) * read_len, pos.reshape(-1).astype(np.uint32), dirs.reshape(-1), length.astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=100_000, help="minimizers of the genome")
    ap.add_argument("--read-len", type=int, default=250, help="minimizers a read")
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--band", type=int, default=62)
    ap.add_argument("--select-coverage", type=int, default=20)
    a = ap.parse_args()
    from metamdbg_amd import capi
    ctx = capi.Context(0)
    mins, off, pos, dirs, lens = synthetic_reads(a.genome, a.read_len, a.coverage, 42)
    m = ctx.minimizers_with_strands(mins, off, pos, dirs, lens)
    n_reads, n_min = len(off) - 1, len(mins)
    print(f"genome {a.genome} minimizers, {n_reads} reads x {a.read_len} minimizers ({a.coverage:.0f}-fold), band {a.band}; {a.runs} timed runs")
    ix = ctx.map_index_build(m)
    an = ctx.map_anchors(ix, m, 0, 3, band=a.band)
    ch = ctx.map_chains(an, a.band)
    sel = ctx.map_select(ch, a.select_coverage)
    for o in (ch, an, ix):
        o.free()
    n_rows = sel.info()["n_selected"]
    print(f"selection: {n_rows} rows for {n_reads} targets at coverage {a.select_coverage}")

    timers = ("verify_join", "radix_sort", "verify_chains", "verify_rows")
    first = ctx.map_verify(sel, m, band=a.band)
    ctx.synchronize()
    times = {t: [] for t in timers}
    last = None
    for _ in range(a.runs):
        if last is not None:
            last.free()
        ctx.timing(True)
        ctx.timing_reset()
        last = ctx.map_verify(sel, m, band=a.band)
        ctx.synchronize()
        for t in timers:
            times[t].append(ctx.timing_get(t)[0])
        ctx.timing(False)
    first.free()
    info = last.info()
    rows = last.to_host()["rows"]
    n_anchors = int(rows["n_anchors"].astype(np.int64).sum())
    print(f"verified: {info['n_rows']} rows, {n_anchors} anchors, {info['n_chains']} chains, {info['n_kept']} kept")

    def d2d(nbytes: int) -> float:
        piece = max(min(nbytes, 1 << 30), 1)
        src, dst = ctx.bytes_create(piece), ctx.bytes_create(piece)
        best = None
        for i in range(a.runs + 1):
            t0 = time.perf_counter()
            left = nbytes
            while left > 0:
                ctx.bytes_copy(dst, 0, src, 0, min(piece, left))
                left -= piece
            ctx.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if i and (best is None or dt < best) else best
        src.free(); dst.free()
        return best

    def report(label, ms, alg, items, unit):
        c = d2d(int(alg))
        print(f"{label:28s} " + " ".join(f"{x:9.3f}" for x in ms) + f" ms | {alg / 1e6:10.1f} MB algorithmic = {alg / min(ms) / 1e6:7.1f} GB/s | d2d of as many bytes "
              f"{c:8.3f} ms ({2 * alg / c / 1e6:7.1f} GB/s read + written) | step / d2d {min(ms) / c:6.2f} | {items / min(ms) / 1e3:9.1f} M {unit}/s")
        return min(ms)

    digits = lambda v: (max(int(v), 1).bit_length() + 7) // 8
    passes = 4 + digits(n_reads - 1)
    total = report("join (keys, count, fill)", times["verify_join"], 12 * n_min + n_rows * a.read_len * 2 * (4 + 4 + 8) + 17 * n_anchors, n_anchors, "anchors")
    total += report(f"the lookup's sort ({passes} passes)", times["radix_sort"], passes * 36 * n_min, n_min, "minimizers")
    total += report("chains", times["verify_chains"], 17 * n_anchors + 64 * n_rows, n_rows, "rows")
    total += report("rows", times["verify_rows"], (64 + 4 + 12) * n_rows + 5 * info["n_kept"], n_rows, "rows")
    print(f"all steps {total:.3f} ms: {n_rows / total / 1e3:.2f} M rows/s, {n_anchors / total / 1e3:.1f} M anchors/s")
    last.free(); sel.free(); m.free()
    ctx.close()


if __name__ == "__main__":
    main()
