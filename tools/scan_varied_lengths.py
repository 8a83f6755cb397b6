"""The scan alone on a length-varied synthetic set, the four-wave block kernel against the pre-filtered variant (GPU box):
random bases, read lengths log-uniform between `lo` and `hi` bases (default 1 kb to 60 kb: across the 27 kb up to which a read is the
pre-filtered variant's at density 0.005, so that the longer ones take the four-wave kernel's launch behind it), so that the 16 waves
of a workgroup finish their reads at very different times.

    python tools/scan_varied_lengths.py [reads [reps [lo [hi]]]]
  Prints one JSON line per setting of "scan_prefilter":
the best and all of `reps` timings of the "scan" timer, the kernel that ran (mdbg_scan_info) and the minimizers found."""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from metamdbg_amd import capi

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
lo = float(sys.argv[3]) if len(sys.argv) > 3 else 1000.0
hi = float(sys.argv[4]) if len(sys.argv) > 4 else 60000.0
rng = np.random.default_rng(42)
lens = np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(np.uint32)
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
reads = ctx.reads_from_packed(words, woff, lens)
ctx.timing(True)
for pf in (0, 1, 0, 1):
    ctx.set_option("scan_prefilter", pf)
    ms, found = [], 0
    for i in range(reps + 1):
        ctx.timing_reset()
        m = ctx.scan(reads, K=15, density=0.005, hpc=True, apply_read_filters=True)
        found = m.info()["n_minimizers"]
        m.free()
        if i:
            ms.append(round(ctx.timing_get("scan")[0], 3))
    print(json.dumps({"scan_prefilter": pf, "reads": n, "bases": int(lens.sum()), "lengths": [int(lo), int(hi)], "reads_27142_up": int((lens >= 27142).sum()), "scan_ms_best": min(ms), "scan_ms": ms,
                      "minimizers": int(found), "last_prefiltered": ctx.scan_info()["last_prefiltered"], "launches": [ctx.scan_info()["prefiltered_launches"], ctx.scan_info()["block_launches"]]}), flush=True)
