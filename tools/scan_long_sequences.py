"""The scan alone on long sequences, with and without "scan_segments" (GPU box): random bases in

    long      2 000 reads x 500 kb, read filters on                 (ultra-long reads: automatic mode cuts them)
    long-q    the same with qualities
    contigs   64 sequences x 5 Mb, no_end_trim = 1, apply_read_filters = 0      (the N4 callers' configuration)
    varied    1 M reads, lengths log-uniform over 1 - 60 kb          (tools/scan_varied_lengths.py's set: forced mode 2 against automatic)

    python tools/scan_long_sequences.py SET [reps [segments [segment_bases [scale]]]]
segments: the value of "scan_segments" (default: the library's own; a library without the option runs as it is and says so);
scale divides the number of sequences (a quick look).  Prints one JSON line: all `reps` timings of the "scan" timer (every launch of a
scan kernel, re-runs of outgrown reads included), of "scan_segments" (the pre-pass and the join) and of the whole mdbg_scan call on the
host's clock, the kernels that ran (mdbg_scan_info) and the minimizers found.  MDBG_LIB selects the library (a parent commit's build)."""
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from metamdbg_amd import capi

which = sys.argv[1] if len(sys.argv) > 1 else "long"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
segments = int(sys.argv[3]) if len(sys.argv) > 3 else None
segment_bases = int(sys.argv[4]) if len(sys.argv) > 4 else 0
scale = int(sys.argv[5]) if len(sys.argv) > 5 else 1
rng = np.random.default_rng(42)
if which in ("long", "long-q"):
    lens = np.full(2000 // scale, 500_000, dtype=np.uint32)
elif which == "contigs":
    lens = np.full(max(1, 64 // scale), 5_000_000, dtype=np.uint32)
elif which == "varied":
    lens = np.exp(rng.uniform(np.log(1000.0), np.log(60000.0), 1_000_000 // scale)).astype(np.uint32)
else:
    raise SystemExit("SET: long, long-q, contigs or varied")
n = len(lens)
units = (lens.astype(np.uint64) + np.uint64(63)) // np.uint64(64)
woff = np.concatenate([[0], np.cumsum(units * np.uint64(2))]).astype(np.uint64)
words = rng.integers(0, 1 << 63, int(woff[-1]), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, int(woff[-1]), dtype=np.uint64)
# zero bases behind every read's last one (the layout of synth.pack_reads)
last = woff[:-1] + (lens.astype(np.uint64) - np.uint64(1)) // np.uint64(32)
rem = (lens % 32).astype(np.uint64)
mask = np.where(rem == 0, np.uint64(0xFFFFFFFFFFFFFFFF), (np.uint64(1) << (np.uint64(2) * rem)) - np.uint64(1))
words[last] &= mask
spare = last + np.uint64(1) < woff[1:]
words[(last + np.uint64(1))[spare]] = 0
ctx = capi.Context(0)
if which == "long-q":
    qoff = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))]).astype(np.uint64)
    quals = (rng.integers(5, 45, int(qoff[-1]), dtype=np.uint8) + np.uint8(33)).tobytes()
    reads = ctx.reads_from_packed_async(words, woff, lens, quals, qoff)
    reads.wait()
else:
    reads = ctx.reads_from_packed(words, woff, lens)
option = "library default"
if segments is not None:
    try:
        ctx.set_option("scan_segments", segments)
        ctx.set_option("scan_segment_bases", segment_bases)
        option = segments
    except capi.MdbgError:
        option = "unknown to this library"
ctx.timing(True)
kw = dict(apply_read_filters=False, no_end_trim=True) if which == "contigs" else dict(apply_read_filters=True)
scan_ms, seg_ms, call_ms, found = [], [], [], 0
for i in range(reps + 1):
    ctx.timing_reset()
    t0 = time.perf_counter()
    m = ctx.scan(reads, K=15, density=0.005, hpc=True, **kw)
    t1 = time.perf_counter()
    found = m.info()["n_minimizers"]
    m.free()
    if i:
        scan_ms.append(round(ctx.timing_get("scan")[0], 3))
        seg_ms.append(round(ctx.timing_get("scan_segments")[0], 3))
        call_ms.append(round((t1 - t0) * 1e3, 3))
info = ctx.scan_info()
print(json.dumps({"set": which, "scan_segments": option, "segment_bases": segment_bases or "default", "sequences": n, "bases": int(lens.astype(np.uint64).sum()),
                  "scan_ms": scan_ms, "scan_segments_ms": seg_ms, "scan_plus_segments_ms_best": round(min(a + b for a, b in zip(scan_ms, seg_ms)), 3),
                  "call_ms": call_ms, "minimizers": int(found), "reads_segmented": info.get("reads_segmented", 0),
                  "last_prefiltered": info["last_prefiltered"], "launches": [info["prefiltered_launches"], info["block_launches"]]}), flush=True)
