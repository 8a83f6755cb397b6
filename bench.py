#!/usr/bin/env python3
"""bench.py -- Gbp/s through the minimizer + k-min-mer step on MI355X (BASELINE.json metric).

A step = one pass of the hot path over one batch of synthetic HiFi reads already resident in HBM
(2-bit packed): reads -> minimizers (HPC, l=15, density 0.005) -> palindrome purge -> k-min-mer
table at k=4 (count + rescue).  N=1 workload = the headline of BASELINE.json's north_star: 10 M x 10 kb
reads (100 Gbp, 25 GB packed) in one batch; N>1: 5 M reads per rank (configs[4]: 40 M reads over 8 ranks).
Two batches are in flight per GPU (--in-flight): consecutive steps run on their own library contexts
(own HIP stream, memory pool and host thread each) over the one resident read set, so the memory-bound table
kernels and the exchanges of one batch overlap the ALU-bound scan of another; every step is still a complete
pass over its batch.  (Three until round 3, when the one-table first pass took a quarter of a step; with the
partitioned pass -- a seventh -- a third batch only adds contention: 840 against 828 Gbp/s, tools/overlap_matrix.sh.)
N>1: one process per GPU, every rank owns its own shard of the same size (weak scaling); only the
k-min-mer counts are global: rows go to their owner rank and the global counts come back, two
all-to-alls inside the library (include/mdbg_hip.h mdbg_comm_create_mode, mdbg_shard_exchange) -- by default ("auto") as PEER COPIES
over xGMI between staging buffers the ranks share (owners pull their slices device to device, hand-shakes through shared host memory:
no collective kernel has to find room beside a scan), after a self-test every rank passed; otherwise RCCL send / receive groups with
the exchange gate.  MDBG_COMM_MODE=peer|rccl|auto selects; MDBG_BENCH_EXCHANGE=torch moves the bytes with torch.distributed instead.

A plain run (`bench.py --gpus 1 --steps N --warmup W`) does only what the headline needs: it sets up, warms up, times the N steps,
writes the last step's outputs when --dump-outputs DIR is given, and prints the line.  Everything else below -- the CPU baseline,
the parity checks, the self-checks, the kminmer roofline and the legs -- runs only with --full.

--dump-outputs DIR: after the timed steps, what the last timed step computed goes to DIR/<name>.npy (float64, integers split into exact
32-bit halves where they are wider; at N > 1 every rank writes <name>_rank<r>.npy): the k-min-mer table's row count, solid count and
order-independent sums over ALL its rows, a fixed sample of its rows chosen by key and sorted by key, and the minimizers of a fixed,
seeded sample of reads before and after the palindrome purge.  The inputs are seeded, so two builds can be compared output for output.

Prints ONE compact JSON line (rank 0; under 4 KB -- compact_line below; the full result goes to bench_detail.json next to this script
and to stderr) with `roofline` (dominant kernel, HIP-event timed on the library's stream; `traffic` only from a PMC
collection made on this very csrc/scan.hip) and, with --full, `roofline_kminmer` (the table kernels alone: 4 M + 16 I + 20 D bytes, and the atomic-rate
ceiling of the insert), `cpu_baseline` (the reference's own code, oracle/_ref/refdrv, timed on this box's cores on BASELINE.json
configs[1] whole -- 1 M reads, 10 Gbp; `path_only` = up to the moment its tables are on disk) and, at N=1, `parity` (the HIP path's
read_data_init bytes, corrected reads, k-min-mer table and abundance checksum against the reference's files for that whole config, plus
the digests committed under tests/golden/hifi_1m; a mismatch fails the run) and `legs`: `end_to_end` (the C++ tool against the
reference from the same FASTA file), `multik` (configs[2]: k = 4..11 over the resident batch, benchmark mode), `multik_reference`
(configs[2] in the reference's own mode: its graph -> contig -> toMinspace loop on 200 000 reads, mdbg_tool graph's tables against the
reference's at every k), `pcie` (reads arriving over the link, synchronous and pipelined) and `ont` (configs[3] at its stated size: 10 M
x 20 kb reads with qualities in three resident pieces, parity on a 100 000-read sample).
At N>1 with --full the line carries a `parity` block too: one more sharded step, its per-rank tables reduced to counts and order-independent sums,
all-reduced and compared with the single-GPU first pass over ALL the reads that rank 0 runs alone; `config.exchange` reports the
communicator's rank count, wire bytes and exchange time per step.  A mismatch fails the run.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# HIP multiplexes streams onto a few hardware queues (4 by default).  With 4, the streams of the two library contexts
# ended up on one queue in every run under torch.distributed + RCCL (no overlap of the batches in flight); with 8 they
# rarely do, and main() checks and repairs the rest.  Must be set before HIP starts.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md
CAND_CYCLES_4, CAND_CYCLES_5 = 160.0, 156.0     # cycles per 64 candidate tests per SIMD at 4 / 5 waves (profiles/round6_n_hash_rates_with_the_merged_candidate_test.txt)
K_MINIMIZER, DENSITY, KMINMER = 15, 0.005, 4
DEFAULT_TABLE_GRID = 0         # workgroups of the kernels that walk every k-min-mer instance, batches in flight (0: one per CU)
DEFAULT_TABLE_CUS = 0          # compute units the table kernels of a batch in flight are confined to (0: not confined)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="reads per GPU per step (10 kb each); default 10 M at N=1, 5 M per rank at N>1")
    ap.add_argument("--total-reads", type=int, default=0, help="strong scaling: ONE read set of this many reads split over the ranks (BASELINE.json configs[4] as north_star "
                                                                "words it: 40 M reads at 1 / 2 / 4 / 8 GPUs); overrides --reads, the line says \"scaling\": \"strong\"")
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--in-flight", type=int, default=2, help="batches processed concurrently per GPU (own context, stream and host thread each)")
    ap.add_argument("--full", action="store_true",
                    help="also the checks and side measurements after the timed steps: kminmer roofline, self-checks, CPU baseline, parity, legs "
                         "(N=1), the single-GPU parity pass (N>1); a plain run only times the headline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (float64; a fixed sample of the table, all of its sums)")
    ap.add_argument("--cpu-sample", type=int, default=1_000_000,
                    help="--full: reads of the CPU-baseline / parity read set, a HiFi set of its own at 50x (1 M = BASELINE.json configs[1]; 0 = skip)")
    ap.add_argument("--legs", default="all", help="--full, N=1 only: comma list of end_to_end,multik,multik_reference,pcie,ont,graph_per_k ('all', 'none')")
    ap.add_argument("--multik-sample", type=int, default=200_000, help="reads of the multik_reference leg (the reference's own loop k = 4..11)")
    ap.add_argument("--ont-reads", type=int, default=10_000_000, help="reads (20 kb, with qualities) of the ont leg: BASELINE.json configs[3]")
    ap.add_argument("--ont-sample", type=int, default=100_000, help="reads of the ont leg's parity sample against the reference")
    ap.add_argument("--detail", default=os.path.join(ROOT, DETAIL_FILE), help="where the full result goes (the stdout line is its compact form)")
    a = ap.parse_args()
    if a.total_reads > 0:
        a.reads = a.total_reads // max(1, a.gpus)          # (a remainder of fewer reads than ranks is left out)
    if a.reads <= 0:
        a.reads = 10_000_000 if a.gpus <= 1 else 5_000_000
    return a

import bench_legs
from bench_legs import (  # noqa: F401  (tests and tools reach these through `bench`)
    ATOMIC_RATE_GOPS, REFDRV, TOOL, _PHASE, _add_summaries, _cores_used, _cpu_quota, _fbytes, _make_tmp, _phase, _run_two_commands, _sample_that_fits,
    _table_summary, _tables_equal, _write_fasta_from_device, git_blob_hash, graph_per_k_leg, index_traffic, kminmer_roofline, kminmer_traffic, measured_traffic,
    multik_leg, multik_reference_leg, multik_rooflines, ont_leg, pcie_leg, run_alone, sample_legs, shard_self_check)

LINE_LIMIT = 4096               # bytes of the one stdout line; the driver's record keeps an 8 KB tail and parses the line out of it
DETAIL_FILE = "bench_detail.json"


def _num(x, digits: int = 6):
    """Numbers of the compact line: six significant digits for floats, everything else as it is."""
    if isinstance(x, bool) or not isinstance(x, float):
        return x
    return float(f"{x:.{digits}g}")


def _pick(src, keys) -> dict:
    src = src or {}
    return {k: _num(src[k]) for k in keys if k in src}


def _short(text, limit: int = 200):
    if not isinstance(text, str) or len(text) <= limit:
        return text
    return text[: limit - 3] + "..."


def _flag(block, key="all_equal"):
    """The boolean a check ended with: None when the check was not made (leg switched off), False when it broke."""
    if not isinstance(block, dict):
        return None
    if "error" in block:
        return False
    return block.get(key)


def compact_line(out: dict) -> dict:
    """The ONE line bench.py prints, from the full result: the contract's keys, the rooflines' scalars, the CPU baseline, the parity
    booleans, one boolean per check and one number per leg -- under LINE_LIMIT bytes whatever the legs produced.  Everything else
    (per-k blocks, notes, traces) is the detail file's (DETAIL_FILE, next to this script) and stderr's."""
    cfg = out.get("config") or {}
    line = {k: _num(out.get(k)) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                          "scaling", "vs_baseline", "dtype", "data")}
    c = {"workload": _short(cfg.get("workload"))}
    c.update(_pick(cfg, ("reads_per_gpu", "read_len", "minimizers_per_step", "kminmer_records", "solid", "batches_in_flight", "device", "cus")))
    if cfg.get("scaling_note"):
        c["scaling_note"] = _short(cfg["scaling_note"], 120)
    ex = cfg.get("exchange")
    if ex:
        c["exchange"] = dict(_pick(ex, ("transport", "rccl_ranks", "ranks", "wire_bytes_per_step", "exchange_ms_per_step", "gate")), path=_short(ex.get("path"), 80))
    line["config"] = c
    roof = out.get("roofline") or {}
    r = _pick(roof, ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch", "avg_launch_ms"))
    r["kernel"] = _short(roof.get("kernel"), 60)
    r["valu_floor"] = _pick(roof.get("valu_floor"), ("frac", "floor_ms"))
    line["roofline"] = r
    kroof = out.get("roofline_kminmer")
    if kroof:
        k = _pick(kroof, ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_over_algorithmic"))
        k["kernel"] = _short(kroof.get("kernel"), 60)
        k["algorithmic_bytes_per_launch"] = _num(kroof.get("algorithmic_bytes"))
        k["avg_launch_ms"] = _num(kroof.get("kernel_ms_total"))
        line["roofline_kminmer"] = k
    per_k = (out.get("roofline_index") or {}).get("per_k") or {}
    if per_k:          # every pass of the loop k = 4 .. 11 (configs[2]): kernel ms, fraction of the HBM peak, counter traffic
        line["roofline_index"] = {k: {"ms": _num(v.get("kernel_ms_total"), 4), "frac": _num(v.get("frac"), 3), "traffic": _num(v.get("traffic"), 4)} for k, v in per_k.items()}
    base = out.get("cpu_baseline")
    if base:
        b = _pick(base, ("value", "unit", "cores", "threads", "kind"))
        b["sample"] = _short(base.get("sample"))
        line["cpu_baseline"] = b
    else:
        line["cpu_baseline"] = None
    par = out.get("parity")
    if par:
        p = {k: v for k, v in par.items() if isinstance(v, bool)}
        p.update(_pick(par, ("reads", "error", "skipped")))
        if "against" in par:
            p["against"] = _short(par["against"], 100)
        if isinstance(par.get("golden"), dict):
            p["golden_digests_equal"] = par["golden"].get("digests_equal")
        if "single_gpu_gbps" in par:
            p["single_gpu_gbps"] = _num(par["single_gpu_gbps"])
        line["parity"] = p
    legs = out.get("legs") or {}
    ont = legs.get("ont") or {}
    line["checks"] = {"self_check": _flag(out.get("self_check")),
                      "multik_self_check": _flag(legs["multik"].get("self_check") if isinstance(legs.get("multik"), dict) and "error" not in legs["multik"] else legs.get("multik")),
                      "multik_reference": _flag(legs.get("multik_reference"), "all_tables_equal"),
                      "ont_parity": _flag(ont.get("parity") if "error" not in ont else ont, "table_multiset_equal") if ont else None,
                      "ont_self_check": _flag(ont.get("self_check") if "error" not in ont else ont) if ont else None}
    numbers = {"multik_s": (legs.get("multik") or {}).get("seconds"), "multik_gbps": (legs.get("multik") or {}).get("gbps"),      # configs[2] whole: scan + purge + k = 4 .. 11
               "ont_gbps": ont.get("gbps"),
               "pcie_gbps": (legs.get("pcie") or {}).get("packed_one_context_pipelined_gbps"),
               "e2e_gbps": (legs.get("end_to_end") or {}).get("mdbg_tool_gbps"), "e2e_one_process_gbps": (legs.get("end_to_end") or {}).get("asm_step_gbps")}
    line["legs"] = {k: _num(v) for k, v in numbers.items() if v is not None}
    gpk = legs.get("graph_per_k") or {}
    if isinstance(gpk.get("per_k"), dict):      # seconds of one `mdbg_tool graph` process per k, from files, at the headline's read count
        line["legs"]["graph_per_k_s"] = {k: _num(v.get("wall_s"), 3) for k, v in gpk["per_k"].items()}
        line["checks"]["graph_per_k_tables"] = bool(gpk.get("all_tables_equal"))
    failed_legs = sorted(k for k, v in legs.items() if isinstance(v, dict) and "error" in v)
    if failed_legs:
        line["legs"]["errors"] = failed_legs
    if "kernel_ms_per_step" in out:
        line["kernel_ms_per_step"] = {k: _num(v, 4) for k, v in out["kernel_ms_per_step"].items() if v}
    if "speedup_vs_cpu_reference_path_only" in out:
        line["speedup_vs_cpu_reference_path_only"] = _num(out["speedup_vs_cpu_reference_path_only"])
    line["detail"] = DETAIL_FILE
    if len(json.dumps(line)) >= LINE_LIMIT:          # cannot happen with the caps above; if it does the contract's keys still get through
        for k in ("roofline_index", "kernel_ms_per_step", "legs", "checks"):
            line.pop(k, None)
    return line


def emit(out: dict, json_fd: int, detail_path: str | None = None) -> None:
    """Full result to the detail file (--detail; DETAIL_FILE next to this script) and stderr, the compact line -- and nothing else -- to
    the real stdout."""
    full = json.dumps(out)
    detail_path = detail_path or os.path.join(ROOT, DETAIL_FILE)
    try:
        with open(detail_path, "w") as f:
            f.write(full + "\n")
    except OSError as exc:
        print(f"[bench] {detail_path} not written: {exc}", file=sys.stderr)
    print("[bench] full result: " + full, file=sys.stderr, flush=True)
    os.write(json_fd, (json.dumps(compact_line(out)) + "\n").encode())


DUMP_SEED = 0x5EED_2026                 # --dump-outputs: which table rows and which reads are sampled
DUMP_TABLE_ROWS = 1 << 18               # the table's sample holds about this many rows and never more than twice as many (9 float64 each)
DUMP_READ_RANGES, DUMP_READS_PER_RANGE = 64, 64     # minimizers of 64 runs of 64 consecutive reads


def _halves(a):
    """u64 values as exact float64: a trailing axis of (low 32 bits, high 32 bits)."""
    import numpy as np
    a = np.asarray(a, dtype=np.uint64)
    return np.stack([(a & np.uint64(0xFFFFFFFF)).astype(np.float64), (a >> np.uint64(32)).astype(np.float64)], axis=-1)


def _table_sample(table):
    """The rows whose key falls in a fixed, seeded 2^-shift of the key space (the same keys whatever the row order the pass left),
    sorted by key: (lo, hi, abundance, vectors or None, shift)."""
    import numpy as np
    n = table.info()["n_records"]
    shift = 0
    while (n >> shift) > DUMP_TABLE_ROWS:
        shift += 1
    recs, vecs = [], []
    chunk = 1 << 22
    for first in range(0, n, chunk):
        rec, vec = table.to_host_range(first, min(chunk, n - first))
        if shift:
            mixed = (rec["lo"] ^ np.uint64(DUMP_SEED)) * np.uint64(0x9E3779B97F4A7C15)      # (wraps modulo 2^64)
            sel = (mixed >> np.uint64(64 - shift)) == 0
            rec, vec = rec[sel], (vec[sel] if vec is not None else None)
        recs.append(rec)
        if vec is not None:
            vecs.append(vec)
    from metamdbg_amd.formats import ABUNDANCE_DTYPE
    rec = np.concatenate(recs) if recs else np.zeros(0, ABUNDANCE_DTYPE)
    order = np.lexsort((rec["lo"], rec["hi"]))[: 2 * DUMP_TABLE_ROWS]
    vec = np.concatenate(vecs)[order] if vecs else None
    rec = rec[order]
    return rec["lo"], rec["hi"], rec["abundance"], vec, shift


def _read_sample(ctx, m, first_read: int):
    """Minimizers of a fixed, seeded set of read runs of m: (global read indices, CSR offsets, minimizer values)."""
    import numpy as np
    n_reads = m.info()["n_reads"]
    per = min(DUMP_READS_PER_RANGE, n_reads)
    if per == 0:
        return np.zeros(0, np.uint64), np.zeros(1, np.uint64), np.zeros(0, np.uint32)
    runs = n_reads // per
    starts = np.sort(np.random.default_rng(DUMP_SEED).choice(runs, size=min(DUMP_READ_RANGES, runs), replace=False)) * per
    reads, counts, values = [], [], []
    for s in starts:
        part = ctx.minimizers_slice(m, int(s), per)
        h = part.to_host(full=False)
        part.free()
        reads.append(np.arange(s, s + per, dtype=np.uint64) + np.uint64(first_read))
        counts.append(np.diff(h["offsets"].astype(np.int64)))
        values.append(h["minimizers"])
    offsets = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.uint64)
    return np.concatenate(reads), offsets, np.concatenate(values)


def dump_outputs(out_dir: str, kept: dict, first_read: int, rank: int, world: int) -> int:
    """--dump-outputs: what the last timed step computed -- its k-min-mer table (counts and order-independent sums over all rows, a sample of
    rows) and the minimizers of sampled reads before and after the purge -- as float64 .npy files in out_dir.  Frees the step's objects;
    returns the bytes written."""
    import numpy as np
    mins, corr, table = kept["mins"], kept["corr"], kept["table"]
    ctx = mins.ctx
    ti = table.info()
    lo, hi, abundance, vec, shift = _table_sample(table)
    arrays = {"counts": np.array([mins.info()["n_reads"], mins.info()["n_minimizers"], corr.info()["n_minimizers"], ti["n_records"], ti["n_solid"]],
                                 dtype=np.float64),
              "table_checksum": _halves(table.checksum()),
              "table_sample_shift": np.array([shift], dtype=np.float64),
              "table_keys": np.concatenate([_halves(lo), _halves(hi)], axis=1),
              "table_abundance": abundance.astype(np.float64)}
    if vec is not None:
        arrays["table_vectors"] = vec.astype(np.float64)
    reads, offsets, values = _read_sample(ctx, mins, first_read)
    arrays.update(sampled_reads=reads.astype(np.float64), minimizer_offsets=offsets.astype(np.float64), minimizers=values.astype(np.float64))
    _, offsets, values = _read_sample(ctx, corr, first_read)
    arrays.update(purged_minimizer_offsets=offsets.astype(np.float64), purged_minimizers=values.astype(np.float64))
    for o in (table, corr, mins):
        o.free()
    os.makedirs(out_dir, exist_ok=True)
    suffix = f"_rank{rank}" if world > 1 else ""
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + suffix + ".npy"), a)
    return sum(a.nbytes for a in arrays.values())


def _arm_deadline(rank: int, world: int, json_fd: int) -> None:
    """A run that hangs (a collective whose peer never arrives: RCCL with more than one rank has not met hardware yet) must end with a line
    that says so, not with the driver's kill: after MDBG_BENCH_DEADLINE_S seconds (default 1800, 900 for N > 1; 0 = never) every rank dumps its Python
    stacks to stderr, rank 0 writes a JSON line with "value": null and the phase it was in, and the process exits with status 3."""
    # (N > 1 runs have no legs and no CPU baseline: minutes, not the default N = 1 run's quarter of an hour at worst)
    secs = float(os.environ.get("MDBG_BENCH_DEADLINE_S", "1800" if world <= 1 else "900") or 0)
    if secs <= 0:
        return
    import faulthandler
    import threading

    def fire():
        print(f"[bench] rank {rank} of {world}: no result after {secs:.0f} s, phase '{_PHASE[0]}'; giving up", file=sys.stderr, flush=True)
        try:
            faulthandler.dump_traceback(file=sys.stderr, all_threads=True)
        except Exception:
            pass
        if rank == 0:
            line = {"metric": "Gbp/s through minimizer+k-min-mer step; bit-exact k-min-mer table vs ref", "value": None, "unit": "Gbp/s", "n_gpus": world,
                    "higher_is_better": True, "error": f"deadline of {secs:.0f} s passed in phase '{_PHASE[0]}' (MDBG_BENCH_DEADLINE_S)"}
            os.write(json_fd, (json.dumps(line) + "\n").encode())
        os._exit(3)
    t = threading.Timer(secs, fire)
    t.daemon = True
    t.start()


def main() -> None:
    args = parse_args()
    # The one JSON line must be the only thing on stdout: RCCL prints a version banner through C stdio, which a redirected
    # stdout delivers at exit -- after the line.  Everything else that goes to file descriptor 1 is sent to stderr.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    import numpy as np
    import torch
    from metamdbg_amd import capi, synth

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            sys.exit("bench.py --gpus N>1 must be launched with torch.distributed.run (one rank per GPU)")
    _arm_deadline(rank, world, json_fd)
    if os.environ.get("MDBG_BENCH_SHARE_GPU") == "1":      # test hook: every rank on device 0 (multi-rank logic on a 1-GPU box)
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    force_exchange = os.environ.get("MDBG_BENCH_FORCE_EXCHANGE") == "1"    # exercise the sharded path on one GPU
    if world > 1 or force_exchange:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        backend = os.environ.get("MDBG_BENCH_BACKEND", "nccl")   # "gloo": exchanges staged through the host (test hook)
        _phase(f"init_process_group({backend})")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    # IN_FLIGHT batches are processed concurrently, each by its own host thread on its own library context (own HIP
    # stream and memory pool) over its own copy of the reads: the k-min-mer kernels of one batch (bound by the atomic
    # rate) and the gaps between launches overlap with the scan of the other (bound by the vector ALU).  Step i runs
    # on slot i % IN_FLIGHT; every step is still the complete pass over one batch.
    n_slots = max(1, args.in_flight)
    _phase("contexts and the resident read set")
    # beside the other batches' scans the table kernels keep to a small footprint: 1 / 2 / 3 / 4 resident blocks per CU gave
    # 676 / 672 / 657 / 643 Gbp/s on one GPU and 489 / 479 / 463 on the per-rank workload of an 8-GPU job run through
    # the sharded path (profiles/r01g_table_footprint_sweep.txt)
    table_blocks = int(os.environ.get("MDBG_TABLE_BLOCKS_PER_CU", "1")) if n_slots > 1 else 0
    # ... and, optionally, to a few compute units of their own ("table_cu_count", include/mdbg_hip.h): sweep in profiles/
    table_cus = int(os.environ.get("MDBG_BENCH_TABLE_CUS", str(DEFAULT_TABLE_CUS))) if n_slots > 1 else 0
    # ... or to fewer workgroups than there are CUs ("table_grid_blocks")
    table_grid = int(os.environ.get("MDBG_BENCH_TABLE_GRID", str(DEFAULT_TABLE_GRID))) if n_slots > 1 else 0
    slots = []
    # one metagenome for the job (MDBG_BENCH_SPEC_RANKS: test hook, the per-rank workload of an N-rank job on one GPU)
    spec_ranks = int(os.environ.get("MDBG_BENCH_SPEC_RANKS", world))
    spec = synth.hifi_spec(args.reads * spec_ranks, seed=42, read_len=args.read_len, coverage=50.0)
    # one resident read set per GPU (rank r owns reads [r*n, (r+1)*n)), read by every context in flight
    shared_reads = None
    # Several batches in flight: everything a batch runs beside another batch's scan must be able to be RESIDENT beside it, or it waits
    # for whole scan launches (a 24 KB block of purge_fix_kernel once sat out 103 ms; round 4's first runs with the partitioned first
    # pass -- 43 KB blocks -- swung between 830 and 574 Gbp/s).  Five blocks of the scan hold 150 of a CU's 160 KB of LDS, so: the scan
    # leaves 28 KB of every CU's LDS free ("scan_lds_reserve": four blocks of 30 KB padded to 32.5 KB instead of five; alone it costs the
    # scan 1.7 %), and the first pass's kernels take their 24 KB forms ("partition_tile" 2048, "partition_slot_list" 0).
    # tools/overlap_matrix.sh, profiles/round4_*_overlap_matrix.txt.
    shared_opts = {"scan_lds_reserve": int(os.environ.get("MDBG_BENCH_SCAN_LDS_RESERVE", "28672")), "partition_tile": int(os.environ.get("MDBG_BENCH_PARTITION_TILE", "2048")),
                   "partition_slot_list": int(os.environ.get("MDBG_BENCH_PARTITION_SLOT_LIST", "0")),
                   # (buckets of 1024 slots: 24.6 KB; a bucket of 2048 -- what the plan may prefer for many keys per instance -- is 49 KB and would wait)
                   "partition_lds_slots": int(os.environ.get("MDBG_BENCH_PARTITION_LDS_SLOTS", "1024"))} if n_slots > 1 else {}

    def configure_shared(c):
        c.set_option("table_blocks_per_cu", table_blocks)
        if table_cus:
            c.set_option("table_cu_count", table_cus)
        if table_grid:
            c.set_option("table_grid_blocks", table_grid)
        for name, value in shared_opts.items():
            c.set_option(name, value)

    for _ in range(n_slots):
        c = capi.Context(local_rank)
        configure_shared(c)
        if shared_reads is None:
            shared_reads = c.reads_synthetic(spec, first_read=rank * args.reads, n_reads=args.reads)
        slots.append((c, shared_reads))
    # N > 1: the exchange runs inside the library (mdbg_comm_create_mode, mdbg_shard_exchange), one communicator per batch in flight.
    # Which transport is the library's business: MDBG_COMM_MODE = peer | rccl | auto (include/mdbg_hip.h).  "auto" (the default) takes
    # PEER COPIES -- staging buffers shared between the ranks, every owner pulls its slices device to device, hand-shakes through a block
    # of shared host memory: no collective kernel has to find room beside a scan -- after a self-test every rank passed, and RCCL
    # send / receive groups otherwise (all ranks together; the exchange gate below then keeps scans off the device during an exchange).
    # MDBG_BENCH_EXCHANGE=torch moves the bytes with torch.distributed's all_to_all_single instead (a harness path: tests).
    rw = capi.lib().mdbg_row_words(KMINMER)
    exchange_mode = os.environ.get("MDBG_BENCH_EXCHANGE", "library")
    backend_name = os.environ.get("MDBG_BENCH_BACKEND", "nccl")
    comms = None
    comm_note = None
    if world > 1 and exchange_mode != "torch" and os.environ.get("MDBG_COMM_MODE", "auto") == "auto" and os.environ.get("MDBG_BENCH_NO_PROBE") != "1":
        # The peer copies are tried in CHILD processes first (tools/peer_probe.py: a communicator over them, its self-test's pulls across the
        # devices): what the library cannot report as an error code -- a GPU memory access fault on the first pull from a device that cannot be
        # addressed -- then ends a child, not the job, and every rank takes RCCL.  (No multi-GPU box was ever in reach of this repository:
        # the first one to run it should not lose its run to that.)
        _phase("probing the peer copies in child processes")
        hand0 = "cuda" if backend_name == "nccl" else "cpu"
        t = torch.zeros(128, dtype=torch.uint8, device=hand0)
        if rank == 0:
            t.copy_(torch.frombuffer(bytearray(os.urandom(128)), dtype=torch.uint8))
        dist.broadcast(t, 0)
        probe_rc = -1
        try:
            probe_rc = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "peer_probe.py"), str(rank), str(world), str(local_rank)],
                                      env=dict(os.environ, MDBG_PROBE_ID=bytes(t.cpu().numpy().tobytes()).hex(), MDBG_PEER_SETUP_TIMEOUT_S=os.environ.get("MDBG_PEER_SETUP_TIMEOUT_S", "40")),
                                      capture_output=True, timeout=120).returncode
        except Exception as ex:
            print(f"[bench] rank {rank}: the peer-copy probe did not finish: {ex}", file=sys.stderr)
        ok_probe = torch.tensor([1 if probe_rc == 0 else 0], device=hand0)
        dist.all_reduce(ok_probe, op=dist.ReduceOp.MIN)
        if int(ok_probe.item()) == 0:
            os.environ["MDBG_COMM_MODE"] = "rccl"
            comm_note = "the peer-copy probe failed in a child process of some rank: RCCL"
            print(f"[bench] rank {rank}: {comm_note} (this rank's probe ended with {probe_rc})", file=sys.stderr)
    if (world > 1 or force_exchange) and exchange_mode != "torch":
        comms = []
        comm_error = None
        _phase("creating the library's communicators (mdbg_comm_create_mode)")
        hand = "cuda" if (dist is not None and backend_name == "nccl") else "cpu"       # where torch.distributed carries the id
        for c, _ in slots:
            t = torch.zeros(128, dtype=torch.uint8, device=hand)
            if rank == 0:
                try:
                    t.copy_(torch.frombuffer(bytearray(capi.Context.comm_unique_id()), dtype=torch.uint8))
                except Exception as ex:              # no id: every rank will see the zero id and fall back together
                    comm_error = str(ex)
            if dist is not None:
                dist.broadcast(t, 0)
            raw = bytes(t.cpu().numpy().tobytes())
            if comm_error is None and any(raw):
                try:
                    comms.append(c.comm_create(raw, rank, world))
                except Exception as ex:
                    comm_error = str(ex)
            elif comm_error is None:
                comm_error = "no communicator id from rank 0"
            # (round-5 ADVICE) slot by slot: a rank whose create failed must not leave the others attaching to the next slot's communicator alone
            if dist is not None:
                ok_slot = torch.tensor([0 if comm_error else 1], device=hand)
                dist.all_reduce(ok_slot, op=dist.ReduceOp.MIN)
                if int(ok_slot.item()) == 0:
                    comm_error = comm_error or "another rank could not create its communicator"
                    break
        # all ranks or none: a rank without its communicators sends everybody to torch.distributed's all-to-all
        ok = torch.tensor([0 if comm_error else 1], device=hand)
        if dist is not None:
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 0:
            comm_note = (comm_note + "; " if comm_note else "") + f"library exchange unavailable ({comm_error or 'another rank failed'})"
            print(f"[bench] {comm_note}: using torch.distributed", file=sys.stderr)
            for cm in comms:
                cm.destroy()
            comms = None
        else:
            comm_note = "; ".join(sorted({cm.note for cm in comms if cm.note} | ({comm_note} if comm_note else set()))) or None      # ("auto" is decided per communicator)
            if comm_note:
                print(f"[bench] the library's communicators fell back to RCCL: {comm_note}", file=sys.stderr)
    ctx, reads = slots[0]
    info = ctx.device_info()
    n_bases = reads.info()["n_bases"]
    exchange = world > 1 or force_exchange

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    trace = os.environ.get("MDBG_BENCH_TRACE") == "1"
    phases: dict = {}
    # the exchanges of the sharded pass use ONE communicator: they run in global step order on every rank, one at a
    # time (a step's scan is several times longer than its exchange, so the turn-taking costs nothing)
    turn = threading.Condition()
    next_exchange = [0]

    wire = {"to_peers": 0, "exchanges": 0, "ms": 0.0}     # the torch.distributed path's own account (the library keeps its own: mdbg_comm_stats)
    corrupt = [os.environ.get("MDBG_BENCH_CORRUPT_REPLY") == "1"]   # test hook: one wrong global count in the verification step of the last rank
    # test hook MDBG_BENCH_FAIL_RANK=r: rank r fails summing the rows it owns (phase 2 of an exchange) in the verification step -- every rank
    # must hear of it and the job must end, non-zero, instead of the peers waiting for replies that never come
    fail_rank = int(os.environ.get("MDBG_BENCH_FAIL_RANK", "-1"))

    # The exchange gate (N > 1 over RCCL): an exchange does not run beside a scan of another batch of this rank.  RCCL's device kernel
    # (ncclDevKernel_Generic: 248 - 256 VGPRs, 37 664 B of LDS a block -- profiles/round4_g_rccl_device_kernel_resources_gfx950.txt) does
    # not fit what four scan blocks leave of a CU (31 744 B of LDS: DESIGN.md 4.4's residency rule), and the scan's grid keeps every freed
    # place refilled until its last block is out: each of the five RCCL launches of an exchange (two all-gathers of status words, two
    # all-to-alls, one more agreement) would sit out the rest of a scan, one after the other.  So: a batch about to exchange first lets
    # the scans in flight on this rank finish and holds new ones back (the other batches' purge and first-pass kernels go on: their
    # blocks are short-lived); the wire time of a step (a few ms over xGMI) is then exposed instead of hidden, which is the bounded price.
    # MDBG_BENCH_EXCHANGE_GATE=0 / 1 overrides (default: on when the exchange runs over RCCL between more than one rank).
    gate_env = os.environ.get("MDBG_BENCH_EXCHANGE_GATE", "auto")
    over_rccl = (comms is not None and any(cm.mode == "rccl" for cm in comms)) or (comms is None and backend_name == "nccl")
    use_gate = exchange and (gate_env == "1" or (gate_env == "auto" and world > 1 and over_rccl))
    from metamdbg_amd.distributed import ExchangeGate
    gate = ExchangeGate(use_gate)

    def step(slot: int, index: int, collect: bool = False):
        """One pass of the hot path over the resident batch on slot `slot`; collect: also the table's order-independent sums
        (mdbg_table_checksum) -- the verification step after the timed region."""
        ctx, reads = slots[slot]
        with gate.scan():
            mins = ctx.scan(reads, K=K_MINIMIZER, density=DENSITY, hpc=True)
            if use_gate:
                ctx.synchronize()
        corr = ctx.purge_palindromes(mins, 4, 100)
        if not exchange:
            table = ctx.kminmer_count_first(corr, KMINMER, 0)
        else:
            from metamdbg_amd import distributed as D
            tr = [time.perf_counter()] if trace else None
            def mark(name):
                if tr is not None:
                    ctx.synchronize()
                    tr.append(time.perf_counter())
                    phases[name] = phases.get(name, 0.0) + (tr[-1] - tr[-2]) * 1e3
            spoil = collect and corrupt[0] and rank == world - 1
            try:
                sh = ctx.shard_begin(corr, KMINMER, world)
            except Exception:
                # the local half failed: the peers are about to enter the exchange of this step and must not wait for this rank
                with turn:
                    turn.wait_for(lambda: next_exchange[0] >= index)
                try:
                    if comms is not None:
                        comms[slot].abort(ctx)
                    else:
                        D.agree(-1, "before the exchange", device="cuda")
                finally:
                    with turn:
                        next_exchange[0] = index + 1
                        turn.notify_all()
                raise
            mark("begin")
            sent = [int(c) for c in sh.counts]
            with turn:
                turn.wait_for(lambda: next_exchange[0] >= index)
            held = contextlib.ExitStack()       # (after the turn: only the batch whose exchange is next holds the scans back)
            held.enter_context(gate.exchange())
            gate_open = held.close
            if comms is not None:
                try:
                    if spoil:
                        ctx.set_option("test_corrupt_replies", 1)
                    if collect and rank == fail_rank:
                        ctx.set_option("test_exchange_fail_phase", 3)
                    d_glob = sh.exchange(comms[slot])
                    mark("exchange")
                finally:
                    gate_open()
                    with turn:
                        next_exchange[0] = index + 1
                        turn.notify_all()
                table = sh.finish(d_glob, 0)
                sh.free()
                mark("finish")
            else:
                try:
                    t_x = time.perf_counter()
                    D.agree(0, "before the exchange", device="cuda")
                    send = torch.as_tensor(capi.DeviceView(sh.d_rows, (sh.n_rows, rw)), device="cuda") if sh.n_rows else \
                        torch.empty((0, rw), dtype=torch.int64, device="cuda")
                    mine, got = D.exchange_by_owner(send, sent)
                    torch.cuda.current_stream().synchronize()      # not the device: the other slot keeps running
                    mark("all_to_all_rows")
                    def owner_sum():
                        if collect and rank == fail_rank:
                            raise RuntimeError(f"test failure on rank {rank} (MDBG_BENCH_FAIL_RANK)")
                        return sh.reduce(mine.data_ptr(), mine.shape[0])
                    d_reply = D.guarded(owner_sum, "summing the rows it owns", device="cuda")
                    reply = torch.as_tensor(capi.DeviceView(d_reply, (mine.shape[0],)), device="cuda") if mine.shape[0] else \
                        torch.empty((0,), dtype=torch.int64, device="cuda")
                    mark("reduce")
                    glob = D.reply_to_senders(reply, got, sent)
                    if spoil and bool((glob < 0).any()):
                        glob[int((glob < 0).nonzero()[0])] += 1       # a key this rank lists (bit 63): its count is off by one
                    torch.cuda.current_stream().synchronize()
                    mark("all_to_all_reply")
                    wire["to_peers"] += (sum(sent) - sent[rank]) * rw * 8 + (sum(got) - got[rank]) * 8
                    wire["exchanges"] += 1
                    wire["ms"] += (time.perf_counter() - t_x) * 1e3
                finally:
                    gate_open()
                    with turn:
                        next_exchange[0] = index + 1
                        turn.notify_all()
                table = sh.finish(glob.data_ptr(), 0)
                sh.free()
                mark("finish")
        n_min = mins.info()["n_minimizers"]
        ti = table.info()
        if collect:
            ti = dict(ti, sums=table.checksum(), stats=table.stats())
        if index == dump_index:
            kept.update(slot=slot, mins=mins, corr=corr, table=table)      # --dump-outputs: freed after the dump
        else:
            for o in (table, corr, mins):
                o.free()
        return n_min, ti

    results: dict = {}
    errors: list = []
    kept: dict = {}

    def run_steps(slot: int, indices: list):
        try:
            torch.cuda.set_device(local_rank)                  # the current device is per thread
            for i in indices:
                results[i] = step(slot, i)
            slots[slot][0].synchronize()
        except BaseException as exc:                           # surface it in the main thread
            errors.append(exc)
            with turn:
                next_exchange[0] = 1 << 60                     # never block the other slot on a dead one
                turn.notify_all()

    def run_phase(first: int, count: int):
        """Steps first .. first+count-1, step i on slot i % n_slots, the slots concurrently."""
        work = [[i for i in range(first, first + count) if i % n_slots == sl] for sl in range(n_slots)]
        threads = [threading.Thread(target=run_steps, args=(sl, w)) for sl, w in enumerate(work) if w]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise errors[0]

    # warm-up: at least one step per slot (pools, table sizing, RCCL set-up), in whole rounds so that the timed steps
    # start on slot 0
    n_warm = max(args.warmup, n_slots)
    n_warm += (-n_warm) % n_slots
    dump_index = n_warm + args.steps - 1 if args.dump_outputs else -1     # the step whose objects step() keeps for the dump
    _phase("warm-up steps")
    run_phase(0, n_warm)

    # HIP multiplexes streams onto a few hardware queues; when the streams of two contexts land on the same queue their
    # kernels run one after the other and the batches in flight do not overlap at all (GPU_MAX_HW_QUEUES=1 reproduces
    # it: 520 instead of 615 Gbp/s).  Probe it with purely local steps (no collective, every rank decides alone): two
    # concurrent steps must take clearly less than twice one step; if not, give slot 1 a new context -- a new stream --
    # and look again.
    def local_step(slot: int):
        c, r = slots[slot]
        mins = c.scan(r, K=K_MINIMIZER, density=DENSITY, hpc=True)
        corr = c.purge_palindromes(mins, 4, 100)
        t = c.kminmer_count_first(corr, KMINMER, 0)
        for o in (t, corr, mins):
            o.free()
        c.synchronize()

    # Every pair of slots: an idle wave of 20 ms on each stream at once (mdbg_stream_spin).  Streams on different hardware queues finish
    # together (about 20 ms), streams that share a queue one after the other (40 ms): the second context of such a pair is replaced.
    # (Until round 3 the probe timed whole steps; with the scans of different contexts taking turns and the table pass down to a sixth
    # of a step, two overlapping steps take 1.9 x one -- it could no longer tell and replaced contexts that were fine.)
    probe = None
    if n_slots > 1 and args.steps > 1:
        def spin_pair(a, b, us=20000):
            for c in (a, b):
                c.synchronize()
            t = time.perf_counter()
            a.stream_spin(us); b.stream_spin(us)
            a.synchronize(); b.synchronize()
            return (time.perf_counter() - t) * 1e3
        local_step(0)
        probe = {"spin_ms": 20.0, "pairs": {}, "contexts_replaced": 0}
        for sl in range(1, n_slots):
            for attempt in range(4):
                worst = max(spin_pair(slots[o][0], slots[sl][0]) for o in range(sl))
                probe["pairs"][str(sl)] = worst
                if worst < 30.0:
                    break
                c, r = slots[sl]
                c.close()
                slots[sl] = (capi.Context(local_rank), r)
                configure_shared(slots[sl][0])
                probe["contexts_replaced"] += 1
                # (the communicator of a slot belongs to the rank, not to the context: comms[sl] stays)
        for sl in range(n_slots):
            local_step(sl)                                     # pools of the local path
    def exchange_account() -> dict:
        """Bytes this rank put on the wire and the host time it spent inside exchanges so far."""
        if comms is not None:
            st = [cm.stats() for cm in comms]
            return {"to_peers": sum(x["bytes_to_peers"] for x in st), "exchanges": sum(x["exchanges"] for x in st),
                    "ms": sum(x["exchange_ms"] for x in st), "rccl_ranks": st[0]["rccl_ranks"] if st[0]["mode"] == "rccl" else None,
                    "reduce_ms": sum(x["reduce_ms"] for x in st), "wait_ms": sum(x["wait_ms"] for x in st), "host_ms": sum(x["host_ms"] for x in st)}
        return dict(wire, rccl_ranks=None, reduce_ms=None, wait_ms=None, host_ms=None)

    for c, _ in slots:
        c.timing(True)
        c.timing_reset()
    acct0 = exchange_account() if exchange else None
    barrier()
    t0 = time.perf_counter()
    _phase("timed steps")
    run_phase(n_warm, args.steps)
    _phase("after the timed steps (verification, legs)")
    barrier()
    dt = time.perf_counter() - t0
    for c, _ in slots:
        c.timing(False)
    acct1 = exchange_account() if exchange else None
    if args.dump_outputs:
        _phase("writing the outputs of the last timed step")
        t_d = time.perf_counter()
        nbytes = dump_outputs(args.dump_outputs, kept, rank * args.reads, rank, world)
        print(f"[bench] rank {rank}: {nbytes / 1e6:.1f} MB of outputs of the last timed step in {args.dump_outputs} "
              f"({time.perf_counter() - t_d:.2f} s)", file=sys.stderr, flush=True)

    # ---- N > 1: the job checks itself (after the timed region).  One more sharded step on every rank, its share of the table
    # reduced to record count, solid count and the order-independent sums of mdbg_table_checksum (sums[0] is the "Checksum
    # kminmer abundance" the reference logs, graph/CreateMdbg.cpp:3321, :3397); the sums over the ranks must be those of the
    # single-GPU first pass over ALL the reads, which rank 0 then runs alone (N x reads_per_gpu reads: 40 M x 10 kb = 100 GB
    # packed at N = 8, one MI355X holds them).  The union of the shares IS the single-GPU table, so a lost row, a count summed
    # twice or a key listed by two ranks shows here, in the run that is being scored.
    verify = None
    if world > 1 and args.full:
        v_min, v_ti = step(0, n_warm + args.steps, collect=True)
        halves = [v_ti["n_records"], v_ti["n_solid"], v_min] + [h for x in v_ti["sums"] for h in (x & 0xFFFFFFFF, x >> 32)]
        vt = torch.tensor(halves, dtype=torch.int64, device="cuda")
        dist.all_reduce(vt, op=dist.ReduceOp.SUM)
        vt = [int(x) for x in vt.tolist()]
        verify = {"records": vt[0], "solid": vt[1], "minimizers": vt[2],
                  "sums": [(vt[3 + 2 * i] + (vt[4 + 2 * i] << 32)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]}
        # every rank gives the blocks its pools keep for reuse back to the device before rank 0's pass over ALL the reads: nothing on a box
        # with a GPU per rank, but ranks that share one (MDBG_BENCH_SHARE_GPU, the only way this path has ever run) otherwise sit on the memory
        # that pass needs (eight ranks of 2 M reads on one MI355X: "out of memory" in the verification, round 5)
        for c, _ in slots:
            c.set_option("pool_trim", 1)
        torch.cuda.synchronize()
        dist.barrier()
    n_min, ti = results[n_warm + args.steps - 1]
    tmax = torch.tensor([dt], dtype=torch.float64, device="cuda")
    totals = torch.tensor([ti["n_records"], ti["n_solid"]], dtype=torch.int64, device="cuda")   # last step, summed over ranks
    if dist is not None:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(totals, op=dist.ReduceOp.SUM)
    dt = float(tmax.item())

    def timing_get(name):
        tot = [c.timing_get(name) for c, _ in slots]
        return sum(t[0] for t in tot), sum(t[1] for t in tot)

    names = ["scan", "scan_compact", "purge_palindromes", "kminmer_split", "kminmer_insert", "kminmer_rescue", "kminmer_emit", "table_clear", "prefix_scan"]
    if exchange:
        names += ["shard_rows", "shard_reduce", "shard_exchange"]
    ktimes = {k: timing_get(k) for k in names}
    scan_ms, scan_n = ktimes["scan"]
    scan_avg_s = scan_ms / 1e3 / max(scan_n, 1)
    # algorithmic bytes of one scan launch: 0.25 B per base read + 10 B per emitted minimizer
    alg_bytes = 0.25 * n_bases + 10.0 * n_min
    achieved = alg_bytes / scan_avg_s / 1e9 if scan_avg_s > 0 else 0.0
    # compute floor of the reference's algorithm on this part: one Murmur3 per homopolymer-compressed position
    hpc_positions = int(0.75 * n_bases)            # HPC keeps 3/4 of uniform random bases
    clock_hz = (info.get("clock_khz") or 2_400_000) * 1e3       # hipDeviceProp_t::clockRate through the library
    hash_floor_ms = hpc_positions / 64 * 186 / (info["n_cu"] * 4) / clock_hz * 1e3

    # ---- what the exchanges of the timed steps put on the wire (all ranks)
    exch = None
    if exchange:
        et = torch.tensor([acct1["to_peers"] - acct0["to_peers"], acct1["exchanges"] - acct0["exchanges"]], dtype=torch.int64, device="cuda")
        em = torch.tensor([acct1["ms"] - acct0["ms"]], dtype=torch.float64, device="cuda")
        if dist is not None:
            dist.all_reduce(et, op=dist.ReduceOp.SUM)
            dist.all_reduce(em, op=dist.ReduceOp.MAX)
        slot_modes = [cm.mode for cm in comms] if comms is not None else []
        lib_mode = (slot_modes[0] if len(set(slot_modes)) == 1 else "mixed") if comms is not None else None
        exch = {"path": ("library: peer copies (mdbg_shard_exchange, MDBG_COMM_PEER: owners pull their slices device to device)" if lib_mode == "peer"
                         else "library: RCCL send/receive groups (mdbg_shard_exchange, MDBG_COMM_RCCL)" if lib_mode == "rccl"
                         else "library: peer copies on some batches in flight, RCCL on others (see transport_per_slot)" if lib_mode == "mixed"
                         else f"torch.distributed all_to_all_single ({backend_name})"),
                "transport": lib_mode or "torch", "transport_per_slot": slot_modes, "comm_note": comm_note,
                # RCCL ranks: what the library's communicator itself reports (ncclCommCount through mdbg_comm_stats) when the rows travel over
                # it; otherwise the size of torch.distributed's RCCL process group (which then carries barriers and the verification only)
                "rccl_ranks": acct1["rccl_ranks"] if lib_mode in ("rccl", "mixed") else (dist.get_world_size() if dist is not None and backend_name == "nccl" else None),
                "ranks": world,
                "wire_bytes_per_step": int(et[0].item()) / args.steps, "wire_bytes_per_step_per_rank": int(et[0].item()) / args.steps / world,
                "exchanges_timed": int(et[1].item()),
                "exchange_ms_per_step": float(em.item()) / args.steps,
                # rank 0's account of that time (peer copies): the owner's reduction (device work), waiting for its own copies and its peers' phases,
                # and what is left -- the transport's own host time
                "exchange_ms_per_step_rank0": {k: (acct1[k] - acct0[k]) / args.steps for k in ("reduce_ms", "wait_ms", "host_ms")} if acct1.get("host_ms") is not None else None,
                "note": "wire bytes = rows to their owners (24 B each) + one u64 reply per row, other ranks only (a rank's own share is a "
                        "device-to-device copy); exchange_ms = host time inside the exchange call incl. waiting for the slowest rank, "
                        "max over ranks; " + ("an exchange waits for the scans in flight on its rank and holds new ones back (gate: RCCL's "
                        "device kernel does not fit beside the scan's blocks on a CU)" if use_gate else "exchanges overlap the other batches' scans"),
                "gate": use_gate, "gate_wait_ms_per_step_rank0_incl_warmup": gate.waited_ms / max(1, args.steps + n_warm)}

    failed = False
    if rank == 0:
        # ---- N > 1: the single-GPU pass over all N x reads_per_gpu reads, against the summed shares of the verification step
        parity_n = None
        if verify is not None:
            total_reads = args.reads * world
            need = total_reads * args.read_len * 0.40          # packed reads + minimizer rows + table, generously
            if need > 0.8 * info["hbm_bytes"]:
                parity_n = {"skipped": f"{total_reads} reads need about {need / 1e9:.0f} GB on one GPU, more than this one holds"}
            else:
                try:
                    for c, _ in slots[1:]:
                        c.close()                                  # their pools make room
                    run_alone(ctx)
                    t_v = time.perf_counter()
                    allr = ctx.reads_synthetic(spec, first_read=0, n_reads=total_reads)
                    ctx.synchronize()
                    # the pass proper, twice: the first grows the context's memory pools to this size (a cold pass takes three times as
                    # long), the second is what one GPU does with ALL the reads of this job -- the N = 1 point of the same read set
                    t_passes = []
                    for rep in range(2):
                        t_p = time.perf_counter()
                        am = ctx.scan(allr, K=K_MINIMIZER, density=DENSITY, hpc=True)
                        ac = ctx.purge_palindromes(am, 4, 100)
                        at = ctx.kminmer_count_first(ac, KMINMER, 0)
                        ctx.synchronize()
                        t_passes.append(time.perf_counter() - t_p)
                        if rep == 0:
                            for o in (at, ac, am):
                                o.free()
                    t_pass = min(t_passes)
                    one = {"records": at.info()["n_records"], "solid": at.info()["n_solid"], "minimizers": am.info()["n_minimizers"],
                           "sums": list(at.checksum())}
                    for o in (at, ac, am, allr):
                        o.free()
                    flags = {"minimizers_equal": one["minimizers"] == verify["minimizers"], "records_equal": one["records"] == verify["records"],
                             "solid_equal": one["solid"] == verify["solid"], "abundance_checksum_equal": one["sums"][0] == verify["sums"][0],
                             "sum_abundance_equal": one["sums"][1] == verify["sums"][1], "key_sum_equal": one["sums"][2] == verify["sums"][2],
                             "vector_sum_equal": one["sums"][3] == verify["sums"][3]}
                    parity_n = {"mode": f"the {world} ranks' shares of one more sharded step (record count, solid count, the order-independent sums of "
                                        "mdbg_table_checksum, all-reduced) against the single-GPU first pass over all the reads, run by rank 0 "
                                        "after the timed region",
                                "reads": total_reads, **flags, "table_equal": all(flags.values()),
                                "sharded": verify, "single_gpu": one, "single_gpu_seconds": time.perf_counter() - t_v,
                                # one GPU over ALL the reads of this job, one batch, nothing else in flight (scan + purge + table): what the
                                # N ranks' aggregate is to be set against on a strong-scaling curve
                                "single_gpu_pass_seconds": t_pass, "single_gpu_pass_seconds_cold": t_passes[0],
                                "single_gpu_gbps": total_reads * args.read_len / 1e9 / t_pass}
                    failed = not parity_n["table_equal"]
                except Exception as exc:       # the check could not be made (memory on this box): the line says so; a made check that fails is fatal
                    parity_n = {"error": f"{type(exc).__name__}: {exc}", "sharded": verify, "reads": total_reads}
        legs_on = set() if (world > 1 or not args.full or args.legs == "none") else \
            ({"end_to_end", "multik", "multik_reference", "pcie", "ont", "graph_per_k"} if args.legs == "all" else set(args.legs.split(",")))
        # ---- the table kernels on the record (4 M + 16 I + 20 D bytes per k): two steps of this context ALONE on
        # the device, timed by HIP events like the scan -- beside another batch's scan they share the CUs, that is not their speed
        kroof = None
        self_check = None
        if world == 1 and args.full:
            kroof = kminmer_roofline(ctx, reads, args.reads, args.read_len)
            # the timed workload's own table, at its full size: the whole batch against the union of the shares of its halves
            run_alone(ctx)
            sm = ctx.scan(reads, K=K_MINIMIZER, density=DENSITY, hpc=True)
            sc = ctx.purge_palindromes(sm, 4, 100)
            sm.free()
            self_check = shard_self_check(ctx, sc, [KMINMER])
            sc.free()
            chk = self_check["per_k"][str(KMINMER)]
            if chk["records"] != ti["n_records"] or chk["solid"] != ti["n_solid"]:
                self_check["all_equal"] = False
                self_check["timed_steps_table"] = {"records": ti["n_records"], "solid": ti["n_solid"]}
            if not self_check["all_equal"]:
                failed = True
                print(f"[bench] SELF-CHECK FAILURE (the timed workload's table against the shares of its halves): {self_check}", file=sys.stderr)
        side = sample_legs(ctx, min(args.cpu_sample, args.reads), args.read_len, "end_to_end" in legs_on) if world == 1 and args.full else {}
        base = side.get("cpu_baseline")
        legs = {}
        if "end_to_end" in side:
            legs["end_to_end"] = side["end_to_end"]
        def leg(name, fn):
            """A leg that breaks (a resource limit on this box, a time-out of the reference) is reported as such and does not take
            the line down with it; a PARITY failure inside a leg is a SystemExit and does."""
            try:
                run_alone(ctx)
                legs[name] = fn()
            except Exception as exc:
                legs[name] = {"error": f"{type(exc).__name__}: {exc}"}
                print(f"[bench] leg {name} failed: {exc}", file=sys.stderr)
        if "multik" in legs_on:
            leg("multik", lambda: multik_leg(ctx, reads, n_bases))
        if "multik_reference" in legs_on:
            leg("multik_reference", lambda: multik_reference_leg(ctx, min(args.multik_sample, args.cpu_sample), args.read_len))
        if "pcie" in legs_on:
            leg("pcie", lambda: pcie_leg(ctx, reads, spec, local_rank))
        if "graph_per_k" in legs_on:
            # the drop-in as the reference calls it: ONE `graph` process per k, from files, on this very read set (round-5 VERDICT item 3)
            # (the tool's processes share the device with this one: what this process only keeps for reuse goes back first -- with the pools of
            # the earlier legs cached here, the k = 4 process once found so little free that it counted in key groups: 1.0 s instead of 0.4)
            for c, _ in slots:
                c.set_option("pool_trim", 1)
            leg("graph_per_k", lambda: graph_per_k_leg(ctx, args.reads, args.read_len))
        if "ont" in legs_on:
            # the HiFi batch and the other contexts' pools make room first
            for c, _ in slots[1:]:
                c.close()
            reads.free()
            ctx.close()
            octx = capi.Context(local_rank)
            try:
                legs["ont"] = ont_leg(octx, args.ont_reads, sample=min(args.ont_sample, args.cpu_sample))
            except Exception as exc:
                legs["ont"] = {"error": f"{type(exc).__name__}: {exc}"}
                print(f"[bench] leg ont failed: {exc}", file=sys.stderr)
            octx.close()
        total_bases = n_bases * world * args.steps
        traffic, traffic_note = measured_traffic(args.reads, args.read_len)
        out = {
            "metric": "Gbp/s through minimizer+k-min-mer step; bit-exact k-min-mer table vs ref",
            "value": total_bases / 1e9 / dt, "unit": "Gbp/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt * 1e3 / args.steps, "higher_is_better": True, "scaling": "strong" if args.total_reads > 0 else "weak", "vs_baseline": None,
            "dtype": "u64", "data": "synthetic",
            # (<= 200 characters: the line's copy is cut there)
            "config": {"workload": f"{args.reads} synthetic HiFi reads x {args.read_len} bp per GPU (seed 42, 0.1% subst., 50x; {n_bases * world / 1e9:.0f} Gbp/step over all GPUs), HPC, "
                                   f"l={K_MINIMIZER}, density {DENSITY}, k={KMINMER} count+rescue; 2-bit packed, resident in HBM",
                       "workload_note": "4 species; one read set per GPU shared by the batches in flight; single k iteration",
                       "reads_per_gpu": args.reads, "read_len": args.read_len, "minimizers_per_step": int(n_min),
                       # (round-5 VERDICT item 10) what "weak" means between this run's N and the N = 1 point of the same curve
                       "scaling_note": ("strong: one read set of --total-reads split over the ranks" if args.total_reads > 0 else
                                        f"weak: {args.reads} reads per GPU at this N; the defaults are 10 M reads at N=1 (the size the metric is quoted on) and 5 M per GPU at N>1 "
                                        "(configs[4]: 40 M over 8), so per-GPU work halves between the N=1 point and the others -- use --reads to hold it fixed"),
                       "kminmer_records": int(totals[0].item()), "solid": int(totals[1].item()),
                       "batches_in_flight": n_slots, "table_blocks_per_cu": table_blocks, "table_grid_blocks": table_grid, "table_cu_count": table_cus, "shared_device_options": shared_opts, "overlap_probe": probe, "device": info["arch"], "cus": info["n_cu"],
                       "exchange": exch, "full": args.full},
            "roofline": {"bound": "valu", "kernel": "scan_fast_kernel<HPC=1,QUAL=0,APPROX=1> (_ZN4mdbg16scan_fast_kernelILb1ELb0ELb1EEEvNS_8ScanArgsE)", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_note,
                         "bound_note": "`achieved` / `peak` / `frac` are the kernel's algorithmic bytes over its launch time against the HBM peak, as the "
                                       "contract defines them; what bounds the kernel is the vector ALU (`valu_floor`), hence \"bound\": \"valu\" (round-3 VERDICT)",
                         "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": scan_avg_s * 1e3,
                         "concurrent_launches": n_slots,
                         "concurrency_note": (f"{n_slots} batches are in flight: a scan launch shares the device with the other batches' "
                                              "table kernels and lasts longer than alone (--in-flight 1 shows it alone); scans of different batches "
                                              "never overlap each other")
                                             if n_slots > 1 else None,
                         "note": "integer-hash kernel: Murmur3_x64_128 of every HPC position (17 integer multiplies at 4.7 cycles per wave64 "
                                 "each; the kernel computes the upper half with the finalisers' last multiplications merged at every position, 14 multiplies, and the full "
                                 "hash of the selected ones) puts the ceiling at the VALU, far below HBM; the PMC counters show the VALU "
                                 "saturated (profiles/r02w_pmc_scan.txt, DESIGN.md 4.1)",
                         # the hash alone, measured in isolation (tools/ubench/hash_rates.hip, profiles/round6_n_hash_rates_with_the_merged_candidate_test.txt):
                         # 186 cycles per 64 full hashes per SIMD at 8 waves, 160 / 156 per 64 candidate tests at 4 / 5 waves
                         # round-5 VERDICT item 7: the floor of the variant that RUNS -- the candidate test (kmer_hash32_hi_merged since round 6: the
                         # finalisers' last multiplications as one; kmer_hash32_hi_nocarry, 168 / 164 cycles, before) at the occupancy in use:
                         # 4 waves per SIMD when the scan leaves room for other batches (scan_lds_reserve), 5 alone -- not the full hash at 8
                         "valu_floor": {"variant": f"kmer_hash32_hi_merged (the candidate test every position takes) at {4 if n_slots > 1 else 5} waves per SIMD",
                                        "cycles_per_64": CAND_CYCLES_4 if n_slots > 1 else CAND_CYCLES_5, "full_hash_cycles_per_64_at_8_waves": 186,
                                        "hpc_positions_per_launch": hpc_positions, "full_hash_floor_ms": hash_floor_ms,
                                        "floor_ms": hash_floor_ms * (CAND_CYCLES_4 if n_slots > 1 else CAND_CYCLES_5) / 186.0,
                                        "frac": hash_floor_ms * (CAND_CYCLES_4 if n_slots > 1 else CAND_CYCLES_5) / 186.0 / (scan_avg_s * 1e3) if scan_avg_s > 0 else None}},
            "kernel_ms_per_step": {k: v[0] / args.steps for k, v in ktimes.items()},
            "cpu_baseline": base,
        }
        if kroof is not None:
            out["roofline_kminmer"] = kroof
        if self_check is not None:
            out["self_check"] = self_check
        if "roofline_per_k" in legs.get("multik", {}):
            out["roofline_index"] = {"per_k": legs["multik"]["roofline_per_k"],
                                     "note": "BASELINE.json configs[2]: every pass of the loop k = 4 .. 11 over the 10 M-read batch, alone on the device (legs.multik)"}
        if "roofline" in legs.get("ont", {}):
            out["roofline_ont"] = legs["ont"]["roofline"]
        if "parity" in side:
            out["parity"] = side["parity"]
        if parity_n is not None:
            out["parity"] = parity_n
        if legs:
            out["legs"] = legs
        if base and base.get("value"):
            out["speedup_vs_cpu_reference_path_only"] = out["value"] / base["value"]
        if trace and phases:
            out["exchange_phase_ms_per_step_incl_warmup"] = {k: v / (args.steps + n_warm) for k, v in phases.items()}
        emit(out, json_fd, args.detail)
    if comms is not None:
        for cm in comms:
            cm.destroy()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if shared_reads.h:
        shared_reads.free()
    for c, _ in slots:
        c.close()
    if failed:
        sys.exit("bench.py: PARITY FAILURE: the ranks' tables do not add up to the single-GPU table (see `parity` in the line above)")


if __name__ == "__main__":
    main()
