#!/usr/bin/env python3
"""The rates of mdbg_spans_extract / mdbg_reads_extract_ranges on one resident batch, from the library's own timers (device events around
the launches): "extract_plan" (ranges, checks, offsets) and "extract_copy" (the gather), beside a device-to-device mdbg_memcpy_device of as
many bytes as the call wrote, timed in the same process -- the yardstick: a copy reads and writes that many bytes and does nothing else.

    python tools/extract_rate.py --reads 1000000 --runs 3

Synthetic HiFi reads (mdbg_reads_synthetic), homopolymer compression, l 15, density 0.005, k 4.  Cases, each in BITSET form (and (c) in
ASCII form as well):
    (a) every window, ENTIRE            (b) every window, LEFT and RIGHT            (c) the reads whole (LoadUnitigsFunctor)
    (d) a skewed batch -- one range of 5 Mb plus 100 000 of 50 bases -- against the same bases in 100 001 equal ranges: the ratio shows
        whether dealing OUTPUT WORDS to the waves keeps one long range from being one wave's work.
ALGORITHMIC bytes: 0.25 B a base read + 0.25 B a base written (1 B written in ASCII form) + 16 B a request.  What the copy moves beyond
that -- a source word fetched by two lanes, offsets and ranges read per word, padding written -- is in its time, not in its bytes.
The first call of every case is a warm-up and is not timed."""
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
    print(f"reads {a.reads} x {a.read_len} bases, {mins.info()['n_minimizers']} minimizers, k {a.k}: {n_win} windows; {a.runs} timed runs a case")
    for name in ("extract_plan", "extract_plan_ranges", "extract_copy"):
        at = ctx.kernel_attributes(name)
        print(f"kernel {name:20s} registers {at['registers']:3d}  scratch {at['scratch']}  static LDS {at['static_lds']}  threads {at['threads']}")

    def case(label: str, call, form: int):
        """call() -> Sequences.  Times `runs` calls by the library's timers and a device-to-device copy of the bytes one call wrote."""
        first = call()                                  # warm-up; kept as the copy's destination
        info = first.info()
        ctx.synchronize()
        plan, copy = [], []
        for _ in range(a.runs):
            ctx.timing(True)
            ctx.timing_reset()
            sq = call()
            ctx.synchronize()
            plan.append(ctx.timing_get("extract_plan")[0])
            copy.append(ctx.timing_get("extract_copy")[0])
            ctx.timing(False)
            if _ < a.runs - 1:
                sq.close()
        dst, src, nbytes = first.device_ptrs()["bytes"], sq.device_ptrs()["bytes"], info["n_bytes"]
        ctx.memcpy_device(dst, src, nbytes)
        d2d = []
        for _ in range(a.runs):
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.memcpy_device(dst, src, nbytes)         # returns when the copy is complete
            d2d.append((time.perf_counter() - t0) * 1e3)
        per_base_out = 1.0 if form == capi.SEQ_ASCII else 0.25
        alg = (0.25 + per_base_out) * info["n_bases"] + 16 * info["n"]
        c, p, d = min(copy), min(plan), min(d2d)
        print(f"{label:44s} {info['n']:9d} requests {info['n_bases'] / 1e6:10.1f} Mbases {nbytes / 1e6:9.1f} MB written | plan "
              + " ".join(f"{x:8.3f}" for x in plan) + " ms | copy " + " ".join(f"{x:8.3f}" for x in copy) + " ms | "
              f"{alg / c / 1e6:7.1f} GB/s of {alg / 1e6:.1f} MB algorithmic (copy), {alg / (c + p) / 1e6:7.1f} GB/s (plan + copy) | d2d of {nbytes / 1e6:.1f} MB "
              + " ".join(f"{x:8.3f}" for x in d2d) + f" ms = {2 * nbytes / d / 1e6:7.1f} GB/s read + written | copy kernel / d2d {c / d:5.2f}")
        sq.close()
        first.close()
        return c

    every = np.arange(n_win, dtype=np.uint64)
    case("(a) every window ENTIRE", lambda: ctx.spans_extract(reads, sp, every, capi.SEQ_ENTIRE), capi.SEQ_BITSET)
    both = np.repeat(every, 2)
    parts = np.tile(np.array([capi.SEQ_LEFT, capi.SEQ_RIGHT], np.uint32), n_win)
    case("(b) every window LEFT and RIGHT", lambda: ctx.spans_extract(reads, sp, both, parts), capi.SEQ_BITSET)
    del both, parts, every
    rd = np.arange(a.reads)
    zero, full = np.zeros(a.reads, np.uint32), np.full(a.reads, a.read_len, np.uint32)
    case("(c) the reads whole, forward", lambda: ctx.reads_extract_ranges(reads, rd, zero, full, zero), capi.SEQ_BITSET)
    case("(c) the reads whole, reversed", lambda: ctx.reads_extract_ranges(reads, rd, zero, full, full), capi.SEQ_BITSET)
    case("(c) the reads whole, forward, ASCII", lambda: ctx.reads_extract_ranges(reads, rd, zero, full, zero, capi.SEQ_ASCII), capi.SEQ_ASCII)
    sp.free(); mins.free(); reads.free()

    # (d) one contig of 5 Mb and reads of 10 kb
    rng = np.random.default_rng(7)
    seqs = [bytes(synth.CODE2ASCII[rng.integers(0, 4, 5_000_000)])] + [bytes(synth.CODE2ASCII[rng.integers(0, 4, 10_000)]) for _ in range(1000)]
    batch = ctx.reads_from_ascii(seqs)
    n_short = 100_000
    r_s = np.concatenate([[0], rng.integers(1, 1001, n_short)])
    st_s = np.concatenate([[0], rng.integers(0, 10_000 - 50, n_short)])
    ln_s = np.concatenate([[5_000_000], np.full(n_short, 50)])
    rv = rng.integers(0, 2, n_short + 1)
    order = rng.permutation(n_short + 1)                 # the long range somewhere among the short
    skew = case("(d) one 5 Mb range + 100 000 of 50 bases", lambda: ctx.reads_extract_ranges(batch, r_s[order], st_s[order], ln_s[order], rv[order]), capi.SEQ_BITSET)
    st_e = rng.integers(0, 5_000_000 - 100, n_short + 1)
    even = case("(d) the same bases in 100 001 ranges of 100", lambda: ctx.reads_extract_ranges(batch, np.zeros(n_short + 1), st_e, np.full(n_short + 1, 100), rv),
                capi.SEQ_BITSET)
    print(f"(d) skewed / equal copy time {skew / even:5.2f}")
    batch.free()
    ctx.close()


if __name__ == "__main__":
    main()
