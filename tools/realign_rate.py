#!/usr/bin/env python3
"""The rates of mdbg_map_realign on one resident batch, from the library's own timers (device events around the launches): "realign_thin"
(the density flag, scan and compaction of the whole set, the backbone), "realign_join" (the lookup's keys, the rows' reads, count and
oriented fill), "radix_sort" (the lookup's sort of the thinned set), "realign_chains", "realign_lists" (fill, normalisation, compaction) --
beside a device-to-device copy of as many bytes as each step's algorithmic bytes, timed in the same process, and beside mdbg_map_verify's
own steps on the same input in the same run: the yardstick, since realign chains about a fifth of the anchors.

    python tools/realign_rate.py --genome 100000 --runs 3

Input: tools/verify_rate.py's (the same generator, the same arguments); the selection is the mapper's own, verified at band 62; the kept
lists are read on the device.  Realign: band 62, density 0.2 (the ratio of the reference's assembly density 0.005 to its correction
density 0.025), min_minimizers 10.
ALGORITHMIC bytes.  thin: per minimizer of the set 10 B read (value, position, direction, quality), 4 B flag and 8 B scan written and read,
10 B a kept minimizer written; 5 B a backbone minimizer read and written.  join: 12 B a thinned minimizer (the lookup written) + per row the
two thinned reads' minimizers (4 B each, twice: count and fill) and the neighbour's lookup (8 B a minimizer, twice) + 17 B an anchor
written.  chains: 17 B an anchor read + 8 B a chain anchor written + 48 B a row written.  lists: 8 B a chain anchor read + 8 B a raw entry
written and read + 14 B a final entry written.  The first call is a warm-up and is not timed.  One run on a shared machine: no spread is
claimed."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from verify_rate import synthetic_reads  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=100_000, help="minimizers of the genome")
    ap.add_argument("--read-len", type=int, default=250, help="minimizers a read")
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--band", type=int, default=62)
    ap.add_argument("--select-coverage", type=int, default=20)
    ap.add_argument("--density", type=float, default=0.2, help="assembly density as a share of the set's")
    a = ap.parse_args()
    from metamdbg_amd import capi
    ctx = capi.Context(0)
    mins, off, pos, dirs, lens = synthetic_reads(a.genome, a.read_len, a.coverage, 42)
    m = ctx.minimizers_with_strands(mins, off, pos, dirs, lens)
    m.attach_qualities(np.random.default_rng(43).integers(0, 41, len(mins)).astype(np.uint8))
    n_reads, n_min = len(off) - 1, len(mins)
    print(f"genome {a.genome} minimizers, {n_reads} reads x {a.read_len} minimizers ({a.coverage:.0f}-fold), band {a.band}, density {a.density}; {a.runs} timed runs")
    ix = ctx.map_index_build(m)
    an = ctx.map_anchors(ix, m, 0, 3, band=a.band)
    ch = ctx.map_chains(an, a.band)
    sel = ctx.map_select(ch, a.select_coverage)
    for o in (ch, an, ix):
        o.free()

    def timed(call, timers):
        first = call()
        ctx.synchronize()
        times, last = {t: [] for t in timers}, None
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

    v, v_times = timed(lambda: ctx.map_verify(sel, m, band=a.band), ("verify_join", "radix_sort", "verify_chains", "verify_rows"))
    vi = v.info()
    v_anchors = int(v.to_host()["rows"]["n_anchors"].astype(np.int64).sum())
    print(f"verified: {vi['n_rows']} rows, {v_anchors} anchors, {vi['n_chains']} chains, {vi['n_kept']} kept")
    r, times = timed(lambda: ctx.map_realign(v, m, 0, 0, a.band, a.density, 10), ("realign_thin", "realign_join", "radix_sort", "realign_chains", "realign_lists"))
    info, h = r.info(), r.to_host()
    rows = h["rows"]
    n_rows, n_entries = info["n_rows"], info["n_entries"]
    n_anchors = int(rows["n_anchors"].astype(np.int64).sum())
    chain = (rows["flags"] & capi.REALIGN_CHAIN) != 0
    n_chain_anchors = int(rows["n_matches"][chain].astype(np.int64).sum())
    n_raw = n_entries                                          # (normalisation erases few entries: the final count stands for the raw one)
    n_backbone = int(h["target_offsets"][-1])
    n_thin = n_backbone                                        # every read is a target: the backbone is the whole thinned set
    print(f"realigned: {n_rows} rows, {int((rows['flags'] & capi.REALIGN_SHORT != 0).sum())} short, {n_anchors} anchors, {info['n_chains']} chains, {n_entries} entries, "
          f"{n_thin} of {n_min} minimizers kept")

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
        print(f"{label:36s} " + " ".join(f"{x:9.3f}" for x in ms) + f" ms | {alg / 1e6:10.1f} MB algorithmic = {alg / min(ms) / 1e6:7.1f} GB/s | d2d of as many bytes "
              f"{c:8.3f} ms | step / d2d {min(ms) / c:6.2f} | {items / min(ms) / 1e3:9.1f} M {unit}/s")
        return min(ms)

    digits = lambda x: (max(int(x), 1).bit_length() + 7) // 8
    passes = 4 + digits(n_reads - 1)
    thin_len = a.read_len * a.density
    total = report("thin (flag, scan, compaction, backbone)", times["realign_thin"], (10 + 2 * 4 + 2 * 8) * n_min + 10 * n_thin + 2 * 5 * n_backbone, n_min, "minimizers")
    total += report("join (keys, count, oriented fill)", times["realign_join"], 12 * n_thin + n_rows * thin_len * 2 * (4 + 4 + 8) + 17 * n_anchors, max(n_anchors, 1), "anchors")
    total += report(f"the lookup's sort ({passes} passes)", times["radix_sort"], passes * 36 * n_thin, n_thin, "minimizers")
    total += report("chains", times["realign_chains"], 17 * n_anchors + 8 * n_chain_anchors + 48 * n_rows, n_rows, "rows")
    total += report("lists (fill, normalise, compact)", times["realign_lists"], 8 * n_chain_anchors + 2 * 8 * n_raw + 14 * n_entries, n_rows, "rows")
    print(f"realign, all steps {total:.3f} ms: {n_rows / total / 1e3:.2f} M rows/s, {n_entries / total / 1e3:.1f} M entries/s")
    v_total = sum(min(v_times[t]) for t in v_times)
    print("verify on the same input: " + ", ".join(f"{t} {min(v_times[t]):.3f} ms" for t in v_times) + f"; all steps {v_total:.3f} ms for {vi['n_rows']} rows, {v_anchors} anchors")
    print(f"realign / verify: {total / v_total:.2f} in time, {n_rows / max(vi['n_rows'], 1):.2f} in rows, {n_anchors / max(v_anchors, 1):.2f} in anchors")
    r.free(); v.free(); sel.free(); m.free()
    ctx.close()


if __name__ == "__main__":
    main()
