"""Regenerates tests/golden/read_select: seeded reads in minimizer space at about 40-fold coverage and what the REFERENCE's read mapper
selects for them -- the per-position heaps of addAlignmentScore fed by its own processAnchors, with the whole set as one chunk and with the
set cut into three chunks, and the chunks' selections merged by its mergeAlignmentScore -- by select_ref.cpp, which is compiled here
against the reference's sources with the flags of tests/golden/read_mapper/make_fixture.py.  No test runs this; only the data it wrote is
read by tests/test_read_select_model.py and tests/test_gpu_read_select.py.

    python tests/golden/read_select/make_fixture.py --ref <path of the reference>

The reads: one random "genome" of 150 u32 minimizers with positions 20 - 60 apart, sampled into about 170 reads of 12 - 60 minimizers (the
sets of tests/golden/read_mapper hold about 3 chains a query: nothing is ever evicted there), half of them on the reverse strand,
positions jittered, 2 % of the minimizers substituted and 2 % dropped -- and every sixth read with 30 % substituted: its chains are sparse,
with scores of zero and below.  A few reads of 0, 5 and 9 minimizers ask nothing.

One configuration per coverage: 20 (the default _usedCoverageForCorrection), 3 and 1, at band 62.  The conditions on the selection are
asserted below by tests/select_model.py, conditions (conditions, not measurements; manifest.json records the counts) -- seeds are tried in
order until the reference's output meets them.

Files: manifest.json, <name>.npz --
  read_offsets, minimizers, positions                        the reads
  cand_query, cand_ref_read, cand_score, cand_n_matches, cand_matches
                                                             every group of 3 anchors or more with a chain, whole set: the candidates
  whole_offsets (reads + 1), whole_ref_read                  the reads selected per query, whole set as one chunk
  chunk_bounds (4), chunk<i>_offsets, chunk<i>_ref_read      the three chunks' read ranges and selections
  merged_offsets, merged_ref_read                            the chunks' selections merged
The arrays manifest.json lists under delta_coded are stored as first differences (tests/select_model.py, load_fixture, sums them up)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
SPANS = os.path.join(os.path.dirname(HERE), "kminmer_spans")
BAND, CHUNKS = 62, 3
CONFIGS = (("coverage20", 20), ("coverage3", 3), ("coverage1", 1))
DELTA_CODED = ("positions", "cand_matches")


def draw_reads(seed: int, genome: int = 150, n_reads: int = 170):
    rng = np.random.default_rng(seed)
    g = rng.integers(1, 1 << 32, genome, dtype=np.uint64).astype(np.uint32)
    gaps = rng.integers(20, 60, genome)
    reads = []
    for r in range(n_reads):
        n = int(rng.integers(12, 61))
        start = int(rng.integers(0, genome - n + 1))
        mins = g[start:start + n].copy()
        gp = gaps[start:start + n] + rng.integers(-3, 4, n)
        sub = rng.random(n) < (0.30 if r % 6 == 5 else 0.02)
        mins[sub] = rng.integers(1, 1 << 32, int(sub.sum()), dtype=np.uint64).astype(np.uint32)
        pos = int(rng.integers(0, 200)) + np.concatenate([[0], np.cumsum(gp[:-1])])
        keep = rng.random(n) >= 0.02
        mins, pos = mins[keep], pos[keep]
        if rng.random() < 0.5:
            mins, pos = mins[::-1], (pos[-1] + int(rng.integers(0, 200))) - pos[::-1]
        reads.append((mins.astype(np.uint32), pos.astype(np.uint32)))
    for n in (0, 5, 9):
        reads.append((g[40:40 + n].copy(), (100 + np.cumsum(gaps[40:40 + n])).astype(np.uint32)))
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def run_reference(exe: str, reads, coverage: int, tmp: str) -> dict:
    text = [str(len(reads))]
    for m, p in reads:
        text.append(" ".join([str(len(m))] + [f"{int(a)} {int(b)}" for a, b in zip(m, p)]))
    out = subprocess.run([exe, str(BAND), str(coverage), str(CHUNKS), tmp], input=("\n".join(text) + "\n").encode(), capture_output=True, check=True).stdout.decode()
    n = len(reads)
    cands, matches, match_offsets = [], [], [0]
    sets = {name: [[] for _ in range(n)] for name in ["whole", "merged"] + [f"chunk{i}" for i in range(CHUNKS)]}
    for line in out.splitlines():
        tag, *f = line.split()
        v = [int(x) for x in f]
        if tag == "G":
            assert v[3] == len(v) - 4
            cands.append(v[:3])
            matches.extend(v[4:])
            match_offsets.append(len(matches))
        elif tag in ("W", "M"):
            assert v[1] == len(v) - 2
            sets["whole" if tag == "W" else "merged"][v[0]] = v[2:]
        elif tag == "K":
            assert v[2] == len(v) - 3
            sets[f"chunk{v[0]}"][v[1]] = v[3:]
    cands = np.array(cands, dtype=np.int64).reshape(-1, 3)
    assert (np.diff(cands[:, 0] * (1 << 32) + cands[:, 1]) > 0).all()          # per query in ascending read order
    offsets = np.concatenate([[0], np.cumsum([len(m) for m, _ in reads])]).astype(np.uint64)
    cat = lambda k: np.concatenate([r[k] for r in reads]).astype(np.uint32)
    data = dict(read_offsets=offsets, minimizers=cat(0), positions=cat(1), cand_query=cands[:, 0].astype(np.uint32), cand_ref_read=cands[:, 1].astype(np.uint32),
                cand_score=cands[:, 2].astype(np.int32), cand_n_matches=np.diff(np.array(match_offsets, np.int64)).astype(np.uint16), cand_matches=np.array(matches, np.uint32),
                chunk_bounds=np.array([c * n // CHUNKS for c in range(CHUNKS + 1)], np.uint32))
    for name, rows in sets.items():
        data[name + "_offsets"] = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
        data[name + "_ref_read"] = np.array([x for r in rows for x in r], np.uint32)
    return data


def conditions(data: dict, coverage: int) -> dict:
    sys.path.insert(0, os.path.dirname(TESTS))
    from tests import select_model as sm
    c = sm.fixture_candidates(data)
    if not np.array_equal(sm.list_scores(c["match_offsets"], c["matches"]), c["score"]):
        raise SystemExit("n_matches - n_diff_query is not 2 n - span")
    if not np.array_equal(sm.marks(c, coverage), sm.fixture_marks(data, c, "whole")):
        raise SystemExit("the model is not the reference")
    parts = sm.fixture_chunks(data, c)
    rows = sm.concat(parts)
    merged = sm.fixture_marks(data, rows, "merged")
    return sm.conditions(c, coverage, parts, merged)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's checkout (holds src/Commons.hpp)")
    ap.add_argument("--first-seed", type=int, default=8100)
    args = ap.parse_args()
    limit = max(os.path.getsize(os.path.join(SPANS, f)) for f in os.listdir(SPANS))
    manifest = dict(delta_coded=list(DELTA_CODED), band=BAND, chunks=CHUNKS, configs=[])
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "select_ref")
        subprocess.run(["g++", "-std=gnu++20", "-O2", "-w", "-fopenmp", "-I" + os.path.join(args.ref, "src"), "-I" + args.ref,
                        os.path.join(HERE, "select_ref.cpp"), os.path.join(args.ref, "src", "utils", "MurmurHash3.cpp"), "-lz", "-o", exe], check=True)
        seed = args.first_seed
        for name, coverage in CONFIGS:
            while True:
                reads = draw_reads(seed)
                data = run_reference(exe, reads, coverage, tmp)
                try:
                    found = conditions(data, coverage)
                    break
                except AssertionError as e:
                    print(name, "seed", seed, "does not meet the conditions:", e)
                    seed += 1
            path = os.path.join(HERE, name + ".npz")
            np.savez_compressed(path, **{k: (np.diff(v.astype(np.int64), prepend=0).astype(np.int32) if k in DELTA_CODED else v) for k, v in data.items()})
            assert os.path.getsize(path) <= limit, (os.path.getsize(path), limit)
            manifest["configs"].append(dict(name=name, coverage=coverage, seed=seed, n_reads=len(reads), n_minimizers=int(data["read_offsets"][-1]),
                                            n_candidates=len(data["cand_query"]), n_matches=len(data["cand_matches"]), n_selected=len(data["whole_ref_read"]),
                                            n_selected_per_chunk=[len(data[f"chunk{i}_ref_read"]) for i in range(CHUNKS)], n_merged=len(data["merged_ref_read"]), **found))
            print(name, "seed", seed, os.path.getsize(path), "bytes of fixture", manifest["configs"][-1])
            seed += 1
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
