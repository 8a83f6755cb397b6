#!/usr/bin/env python3
"""The rates of mdbg_spans_stitch / mdbg_reads_stitch_ranges / mdbg_sequences_to_fasta_bytes on one resident batch, from the library's own
timers (device events around the launches): "stitch_plan" (ranges, checks, two scans), "stitch_copy" (the gather), "fasta_plan",
"fasta_write" -- beside a device-to-device copy of as many bytes as the call wrote, timed in the same process: the yardstick, which reads
and writes that many bytes and does nothing else.

    python tools/stitch_rate.py --reads 1000000 --runs 3

The reads of tools/extract_rate.py: synthetic HiFi reads (mdbg_reads_synthetic), homopolymer compression, l 15, density 0.005, k 4.  Cases:
    (a) one contig a read made of all its windows by the reference's rule: ENTIRE, then RIGHTs
    (b) the same with every second contig flipped (its windows in reverse order, ENTIRE then LEFTs, flip 1)
    (c) one piece a contig, the read whole -- and mdbg_reads_extract_ranges on the same ranges in the same run: that code is the baseline
        the stitch is read against
    (d) one 5 Mb contig of 25 000 pieces plus 100 000 one-piece contigs of 50 bases, against the same bases in 100 001 equal contigs:
        the ratio shows whether dealing OUTPUT WORDS to the waves keeps one long contig from being one wave's work
    and mdbg_sequences_to_fasta_bytes on (a)'s result.
ALGORITHMIC bytes.  The stitch: 0.25 B a base read + 0.25 B a base written (1 B in ASCII form) + 16 B a piece.  The text: 0.25 B a base
read + 1 B a base written.  The first call of every case is a warm-up and is not timed."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--k", type=int, default=4)
    a = ap.parse_args()
    from metamdbg_amd import capi, synth
    ctx = capi.Context(0)
    reads = ctx.reads_synthetic(synth.hifi_spec(a.reads, seed=42, read_len=a.read_len, coverage=50.0))
    assert reads.info()["n_bases"] == a.reads * a.read_len
    mins = ctx.scan(reads, K=15, density=0.005, hpc=True, apply_read_filters=False)
    sp = ctx.kminmer_spans(reads, mins, K=15, hpc=True, k=a.k)
    n_win = sp.info()["n_windows"]
    woff = sp.to_host()["window_offsets"].astype(np.uint64)
    print(f"reads {a.reads} x {a.read_len} bases, {mins.info()['n_minimizers']} minimizers, k {a.k}: {n_win} windows; {a.runs} timed runs a case")
    for name in ("stitch_plan", "stitch_plan_ranges", "stitch_contigs", "stitch_copy", "fasta_plan", "fasta_write"):
        at = ctx.kernel_attributes(name)
        print(f"kernel {name:20s} registers {at['registers']:3d}  scratch {at['scratch']}  static LDS {at['static_lds']}  threads {at['threads']}")

    def timed(call, timers):
        """call() -> object; `runs` calls by the library's timers; returns (first result, last result, [times per timer])."""
        first = call()                                  # warm-up; kept as the copy's destination
        ctx.synchronize()
        times = [[] for _ in timers]
        last = None
        for _ in range(a.runs):
            if last is not None:
                last.free()
            ctx.timing(True)
            ctx.timing_reset()
            last = call()
            ctx.synchronize()
            for t, name in zip(times, timers):
                t.append(ctx.timing_get(name)[0])
            ctx.timing(False)
        return first, last, times

    def d2d(copy):
        copy()
        ctx.synchronize()
        out = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            copy()
            ctx.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    def case(label: str, call, form: int, n_pieces: int, timers=("stitch_plan", "stitch_copy")):
        first, sq, (plan, copy) = timed(call, timers)
        info = first.info()
        dst, src, nbytes = first.device_ptrs()["bytes"], sq.device_ptrs()["bytes"], info["n_bytes"]
        dd = d2d(lambda: ctx.memcpy_device(dst, src, nbytes))
        alg = (0.25 + (1.0 if form == capi.SEQ_ASCII else 0.25)) * info["n_bases"] + 16 * n_pieces
        c, p, d = min(copy), min(plan), min(dd)
        print(f"{label:46s} {info['n']:8d} sequences {n_pieces:9d} pieces {info['n_bases'] / 1e6:9.1f} Mbases {nbytes / 1e6:8.1f} MB written | plan "
              + " ".join(f"{x:8.3f}" for x in plan) + " ms | copy " + " ".join(f"{x:8.3f}" for x in copy) + " ms | "
              f"{alg / c / 1e6:7.1f} GB/s of {alg / 1e6:.1f} MB algorithmic (copy), {alg / (c + p) / 1e6:7.1f} GB/s (plan + copy) | d2d of {nbytes / 1e6:.1f} MB "
              + " ".join(f"{x:8.3f}" for x in dd) + f" ms = {2 * nbytes / d / 1e6:7.1f} GB/s read + written | copy kernel / d2d {c / d:5.2f}")
        sq.free()
        return c, first

    # (a), (b): one contig a read, all its windows
    pieces = np.zeros(n_win, capi.STITCH_PIECE)
    pieces["window"] = np.arange(n_win, dtype=np.uint64)
    pieces["part"] = capi.SEQ_RIGHT
    pieces["part"][woff[:-1][woff[:-1] < woff[1:]]] = capi.SEQ_ENTIRE
    _, result_a = case("(a) a contig a read: ENTIRE, then RIGHTs", lambda: ctx.spans_stitch(reads, sp, pieces, woff), capi.SEQ_BITSET, n_win)
    text, last, (tp, tw) = timed(lambda: ctx.sequences_to_fasta_bytes(result_a), ("fasta_plan", "fasta_write"))
    info = result_a.info()
    scratch = ctx.bytes_create(text.n)
    dd = d2d(lambda: ctx.bytes_copy(scratch, 0, text, 0, text.n))
    alg = 1.25 * info["n_bases"]
    print(f"{'    the text of (a)':46s} {info['n']:8d} sequences {text.n / 1e6:9.1f} MB of text | plan " + " ".join(f"{x:8.3f}" for x in tp) + " ms | write "
          + " ".join(f"{x:8.3f}" for x in tw) + f" ms | {alg / min(tw) / 1e6:7.1f} GB/s of {alg / 1e6:.1f} MB algorithmic (write) | d2d of {text.n / 1e6:.1f} MB "
          + " ".join(f"{x:8.3f}" for x in dd) + f" ms = {2 * text.n / min(dd) / 1e6:7.1f} GB/s read + written | write kernel / d2d {min(tw) / min(dd):5.2f}")
    for o in (text, last, scratch, result_a):
        o.free()
    flipped = np.repeat(np.arange(a.reads) & 1, np.diff(woff.astype(np.int64))).astype(bool)
    mirror = np.repeat(woff[:-1] + woff[1:] - 1, np.diff(woff.astype(np.int64))) - np.arange(n_win, dtype=np.uint64)       # the windows of a read in reverse order
    pieces["window"][flipped] = mirror[flipped]
    pieces["part"][flipped & (pieces["part"] == capi.SEQ_RIGHT)] = capi.SEQ_LEFT
    pieces["flip"] = flipped
    case("(b) ... every second contig flipped", lambda: ctx.spans_stitch(reads, sp, pieces, woff), capi.SEQ_BITSET, n_win)[1].free()
    del pieces, flipped, mirror

    # (c) the reads whole: a contig of one piece, and the extract of the same ranges
    rd = np.arange(a.reads)
    zero, full = np.zeros(a.reads, np.uint32), np.full(a.reads, a.read_len, np.uint32)
    one_each = np.arange(a.reads + 1, dtype=np.uint64)
    for label, rv, form in (("forward", zero, capi.SEQ_BITSET), ("reversed", full, capi.SEQ_BITSET), ("forward, ASCII", zero, capi.SEQ_ASCII)):
        s = case(f"(c) the reads whole, {label}: stitch", lambda: ctx.reads_stitch_ranges(reads, rd, zero, full, rv, one_each, form), form, a.reads)
        s[1].free()
        e = case(f"(c) the reads whole, {label}: extract", lambda: ctx.reads_extract_ranges(reads, rd, zero, full, rv, form), form, a.reads, ("extract_plan", "extract_copy"))
        e[1].free()
        print(f"(c) {label}: stitch copy / extract copy {s[0] / e[0]:5.2f}")
    sp.free(); mins.free(); reads.free()

    # (d) one contig of 5 Mb in 25 000 pieces and 100 000 contigs of one 50-base piece
    rng = np.random.default_rng(7)
    seqs = [bytes(synth.CODE2ASCII[rng.integers(0, 4, 5_000_000)])] + [bytes(synth.CODE2ASCII[rng.integers(0, 4, 10_000)]) for _ in range(1000)]
    batch = ctx.reads_from_ascii(seqs)
    n_short, n_cut = 100_000, 25_000
    at = int(rng.integers(0, n_short))                  # the long contig somewhere among the short
    r = np.concatenate([rng.integers(1, 1001, at), np.zeros(n_cut, np.int64), rng.integers(1, 1001, n_short - at)])
    st = np.concatenate([rng.integers(0, 10_000 - 50, at), np.arange(n_cut) * 200, rng.integers(0, 10_000 - 50, n_short - at)])
    ln = np.concatenate([np.full(at, 50), np.full(n_cut, 200), np.full(n_short - at, 50)])
    rv = rng.integers(0, 2, len(r))
    off = np.concatenate([np.arange(at + 1), at + n_cut + np.arange(n_short - at + 1)]).astype(np.uint64)
    skew = case("(d) one 5 Mb contig of 25 000 pieces + 100 000", lambda: ctx.reads_stitch_ranges(batch, r, st, ln, rv, off), capi.SEQ_BITSET, len(r))
    skew[1].free()
    n_even = n_short + 1
    st_e = rng.integers(0, 5_000_000 - 100, n_even)
    even = case("(d) the same bases in 100 001 contigs of 100", lambda: ctx.reads_stitch_ranges(batch, np.zeros(n_even), st_e, np.full(n_even, 100), rv[:n_even],
                                                                                              np.arange(n_even + 1)), capi.SEQ_BITSET, n_even)
    even[1].free()
    print(f"(d) skewed / equal copy time {skew[0] / even[0]:5.2f}")
    batch.free()
    ctx.close()


if __name__ == "__main__":
    main()
