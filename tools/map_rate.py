#!/usr/bin/env python3
"""The rates of mdbg_map_index_build / mdbg_map_anchors / mdbg_map_chains / mdbg_map_select on one resident batch, from the library's own timers (device
events around the launches): "map_index" (windows, sort, entries, runs), "map_count" + "map_fill" (the join), "radix_sort" (the regrouping
of the anchors), "map_group" (heads, sizes, the final rows), "map_chains" + "map_matches", "map_select" + its "radix_sort" -- beside a device-to-device copy of as many
bytes as each step's algorithmic bytes, timed in the same process: the yardstick, which reads and writes that many bytes and does nothing
else.

    python tools/map_rate.py --genome 100000 --runs 3

Input: a synthetic genome in minimizer space (random u32 minimizers 20 - 60 apart), reads of about 250 minimizers -- 10 kb at the
correction density 0.025 -- at 20-fold coverage, half of them on the reverse strand, 2 % of the minimizers changed; uploaded with their
positions (mdbg_minimizers_from_host + mdbg_minimizers_attach_positions).  The reads are chunk and queries at once, as in ReadMapper's first
chunk; band 62, min_anchors 3.
ALGORITHMIC bytes.  index: 8 B a minimizer read + 25 B an entry written + the sort's passes.  A sort pass: 12 B an item read twice (count,
scatter) + 12 B written.  count + fill: 8 B a query minimizer + 20 B an anchor written.  group: 20 B an anchor read + 21 B written.
chains: 13 B an anchor read + 80 B a pair written + 4 B a match.  select (--coverage, 20): 80 B a pair read + 12 B a candidate's key and
number written + the sort's passes (the query's bytes and one of the score) + 4 B a match read once + 24 B a selected row and 4 B a match of
its list written.  Behind the table: the selected rows against the pairs, and the bytes that cross to the host with the selection (or with
the alignment file alone) against those of the chain rows and their lists.  The first call of every step is a warm-up and is not timed."""
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
    gpos = np.cumsum(rng.integers(20, 60, genome))
    n_reads = int(coverage * genome / read_len)
    start = rng.integers(0, genome - read_len, n_reads)
    at = start[:, None] + np.arange(read_len)[None, :]
    mins, pos = g[at], gpos[at] - gpos[start][:, None] + rng.integers(0, 200, n_reads)[:, None]
    changed = rng.random(mins.shape) < 0.02
    mins[changed] = rng.integers(1, 1 << 32, int(changed.sum()), dtype=np.uint64).astype(np.uint32)
    rev = rng.random(n_reads) < 0.5
    mins[rev] = mins[rev, ::-1]
    pos[rev] = (pos[rev, -1:] + 100) - pos[rev, ::-1]
    return mins.reshape(-1), np.arange(n_reads + 1, dtype=np.uint64) * read_len, pos.reshape(-1).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=100_000, help="minimizers of the genome")
    ap.add_argument("--read-len", type=int, default=250, help="minimizers a read")
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--band", type=int, default=62)
    ap.add_argument("--select-coverage", type=int, default=20, help="coverage of the per-position selection (_usedCoverageForCorrection)")
    a = ap.parse_args()
    from metamdbg_amd import capi
    ctx = capi.Context(0)
    mins, off, pos = synthetic_reads(a.genome, a.read_len, a.coverage, 42)
    m = ctx.minimizers_with_positions(mins, off, pos)
    print(f"genome {a.genome} minimizers, {len(off) - 1} reads x {a.read_len} minimizers ({a.coverage:.0f}-fold), band {a.band}; {a.runs} timed runs a step")
    for name in [n for n in ctx.step_kernel_names() if n.startswith(("map_", "sort_", "select", "verify"))]:
        at = ctx.kernel_attributes(name)
        print(f"kernel {name:18s} registers {at['registers']:3d}  scratch {at['scratch']}  static LDS {at['static_lds']:6d}  threads {at['threads']}")

    def timed(call, timers):
        first = call()
        ctx.synchronize()
        times = {t: [] for t in timers}
        last = None
        for _ in range(a.runs):
            if last is not None:
                last.free()
            ctx.timing(True)
            ctx.timing_reset()
            last = call()
            ctx.synchronize()
            for t in timers:
                times[t].append(ctx.timing_get(t)[0])
            ctx.timing(False)
        first.free()
        return last, times

    def d2d(nbytes: int) -> float:
        """ms of the fastest of `runs` device-to-device copies of nbytes (in pieces of at most 1 GB)"""
        piece = min(nbytes, 1 << 30)
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

    n_min = len(mins)
    ix, t = timed(lambda: ctx.map_index_build(m), ("map_index", "radix_sort"))
    info = ix.info()
    n_e = info["n_entries"]
    print(f"index: {n_e} entries, {info['n_pairs']} distinct pairs, longest run {info['longest_run']}; its sort " + " ".join(f"{x:.3f}" for x in t["radix_sort"]) + " ms")
    digits = lambda v: (max(int(v), 1).bit_length() + 7) // 8       # the sort's passes: the key's bytes that differ
    total = report("index (with its sort)", t["map_index"], 8 * n_min + 25 * n_e + 8 * 36 * n_e, n_e, "entries")

    an, t = timed(lambda: ctx.map_anchors(ix, m, 0, 3, band=a.band), ("map_count", "map_fill", "radix_sort", "map_group"))
    ai = an.info()
    n_a = ai["n_anchors"]
    print(f"anchors: {n_a} in {ai['n_pairs']} pairs of 3 or more, longest pair {ai['longest_pair']}")
    join = [x + y for x, y in zip(t["map_count"], t["map_fill"])]
    total += report("count + fill", join, 8 * n_min + 20 * n_a, n_a, "anchors")
    sort_passes = digits(n_e - 1) + digits(len(off) - 2)
    sort_ms = report(f"sort of the anchors ({sort_passes} passes)", t["radix_sort"], sort_passes * 36 * n_a, n_a, "anchors")
    total += sort_ms
    total += report("group + final rows", t["map_group"], 41 * n_a, n_a, "anchors")

    ch, t = timed(lambda: ctx.map_chains(an, a.band), ("map_chains", "map_matches"))
    ci = ch.info()
    chain_ms = [x + y for x, y in zip(t["map_chains"], t["map_matches"])]
    total += report("chains + match lists", chain_ms, 13 * n_a + 80 * ci["n_pairs"] + 4 * ci["n_matches"], ci["n_pairs"], "pairs")
    print(f"chains: {ci['n_chains']} of {ci['n_pairs']} pairs, {ci['n_matches']} matches; the timer map_chains alone " + " ".join(f"{x:.3f}" for x in t["map_chains"]) + " ms")
    print(f"all steps {total:.3f} ms: {n_a / total / 1e3:.1f} M anchors/s, {ci['n_pairs'] / total / 1e3:.2f} M pairs/s; the anchors' sort is {100 * sort_ms / total:.0f} % of it")

    sel, t = timed(lambda: ctx.map_select(ch, a.select_coverage), ("map_select", "radix_sort"))
    si = sel.info()
    n_q, n_c, n_s = si["n_queries"], si["n_candidates"], si["n_selected"]
    rank_passes = digits(n_q - 1) + 1
    select_ms = [x + y for x, y in zip(t["map_select"], t["radix_sort"])]
    best = report(f"select ({rank_passes} passes of its sort)", select_ms, 80 * ci["n_pairs"] + 12 * n_c + rank_passes * 36 * n_c + 4 * ci["n_matches"] + 24 * n_s + 4 * si["n_matches"],
                  n_c, "candidates")
    mean_list = ci["n_matches"] / max(n_c, 1)
    trips = max(1, -(-int(round(mean_list)) // 64))
    print(f"select: the timer map_select alone " + " ".join(f"{x:.3f}" for x in t["map_select"]) + " ms, its sort " + " ".join(f"{x:.3f}" for x in t["radix_sort"]) + f" ms; against the chains step of this run: {best / min(chain_ms):.2f}; "
          f"mean list {mean_list:.1f} matches = {100 * mean_list / (64 * trips):.0f} % of the lanes of its {trips} trip(s)")
    by = ctx.selection_to_alignment_bytes(sel)
    chain_bytes = 8 * (n_q + 1) + 80 * ci["n_pairs"] + 8 * (ci["n_pairs"] + 1) + 4 * ci["n_matches"]
    sel_bytes = 8 * (n_q + 1) + 24 * n_s + 8 * (n_s + 1) + 4 * si["n_matches"]
    print(f"selected: {n_s} rows of {n_c} candidates of {ci['n_pairs']} pairs ({100 * n_s / max(ci['n_pairs'], 1):.1f} %) at coverage {a.select_coverage}")
    print(f"to the host: chain rows + lists {chain_bytes / 1e6:.2f} MB; the selection with its lists {sel_bytes / 1e6:.2f} MB ({100 * sel_bytes / chain_bytes:.1f} %); "
          f"the alignment file alone {by.n / 1e6:.2f} MB ({100 * by.n / chain_bytes:.1f} %)")
    by.free(); sel.free()
    for o in (ch, an, ix, m):
        o.free()
    ctx.close()


if __name__ == "__main__":
    main()
