"""Regenerates tests/golden/read_verify: seeded reads in minimizer space with positions, directions and raw lengths, a selection of
neighbours per target, and what the REFERENCE's MinimizerChainer::computeChainingAlignment and the four tests of filterAlignments
(ReadCorrection.hpp:5088-5094) give for every (target, neighbour) row -- by verify_ref.cpp, which is compiled here against the reference's
sources with the language level, include paths and -fopenmp of oracle/Makefile's REF_FLAGS, but at -O2 and without -ffunction-sections
-fdata-sections (as tests/golden/read_mapper does; the driver's arithmetic is integer but for the identity, which tests/host/test_verify.cpp
reproduces bit for bit at -O1).  No test runs this; only the data it wrote is read by tests/test_read_verify_model.py,
tests/test_verify_host.py and tests/test_gpu_read_verify.py.

    python tests/golden/read_verify/make_fixture.py --ref <path of the reference>

The reads: the genomes of the read_mapper generator (tandem repeats, runs of one minimizer, shared segments at other spacings, inverted
copies), every genome minimizer with a strand bit, sampled into 250 reads of 0 - 600 minimizers (the reads of 0 and 1 minimizers are there on purpose), half of them reverse-complemented
(the order turned round, positions counted from the other end, directions flipped).  Substitution and drop rates: 1 % and 6 %, and -- so
that identities fall on both sides of the threshold, which at 0.96 and size 15 is n_matches / n_seeds = 0.54 -- noisy reads at 10 - 45 %.
Chimeric reads (two pieces of genome one behind the other) give chains that end inside both reads: overhangs above the limit.  Per target the
selection lists up to 8 of the reads that share a minimizer with it, and now and then one that shares none.

One configuration per band: 62 (min_identity 0.96f, minimizer_size 15), 5 (0.96f, 13) and 100 (0.9f, 15).  The conditions on the rows are
asserted below (conditions, not measurements; manifest.json records the counts) -- seeds are tried in order until the reference's output
meets them.

Files: manifest.json, <name>.npz --
  read_offsets, minimizers, positions, directions, read_lengths      the reads
  sel_offsets (targets + 1; target t is read t), sel_neighbour       the selection's rows
  row_n_anchors, row_chain, row_<field>, row_identity (float32), row_kept      per row what the reference computed (zeros where there is no chain)
The arrays manifest.json lists under delta_coded are stored as first differences (tests/verify_model.py, load_fixture, sums them up)."""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(TESTS))
from tests import verify_model as vm  # noqa: E402

_spec = importlib.util.spec_from_file_location("read_mapper_fixture", os.path.join(os.path.dirname(HERE), "read_mapper", "make_fixture.py"))
rm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rm)

CONFIGS = (dict(name="band62", band=62, max_overhang=1000, min_overlap_length=1000, min_identity=0.96, minimizer_size=15),
           dict(name="band5", band=5, max_overhang=1000, min_overlap_length=1000, min_identity=0.96, minimizer_size=13),
           dict(name="band100", band=100, max_overhang=1000, min_overlap_length=1000, min_identity=0.9, minimizer_size=15))
DELTA_CODED = ("positions", "sel_neighbour", "row_reference_start", "row_reference_end", "row_query_start", "row_query_end")
ROW_FIELDS = ("n_anchors", "chain", "query_reversed", "n_matches", "n_mismatches", "n_deletions", "n_insertions", "identity_bits", "overhang_start", "overhang_end",
              "align_length", "reference_start", "reference_end", "query_start", "query_end", "kept")
SIZE_LIMIT = 128918          # the largest fixture file the suite had before this one (tests/golden/kminmer_spans)


def sample(rng, pieces, reverse, rate, jitter=3):
    """pieces: [(minimizers, gaps, strands), ...] laid one behind the other -> (minimizers, positions, directions, raw length)"""
    m = np.concatenate([p[0] for p in pieces]).astype(np.uint32)
    g = np.concatenate([p[1] for p in pieces]).astype(np.int64)
    d = np.concatenate([p[2] for p in pieces]).astype(np.uint8)
    n = len(m)
    if jitter:
        g = g + rng.integers(-jitter, jitter + 1, n)
    sub = rng.random(n) < rate
    m[sub] = rng.integers(1, 1 << 32, int(sub.sum()), dtype=np.uint64).astype(np.uint32)
    d[sub] = rng.integers(0, 2, int(sub.sum())).astype(np.uint8)
    pos = int(rng.integers(0, 200)) + np.concatenate([[0], np.cumsum(g[:-1])]) if n else np.zeros(0, np.int64)
    keep = rng.random(n) >= rate
    m, pos, d = m[keep], pos[keep], d[keep]
    length = (int(pos[-1]) if len(pos) else 0) + int(rng.integers(15, 200))
    if reverse:
        m, pos, d = m[::-1], length - 1 - pos[::-1], (1 - d[::-1]).astype(np.uint8)
    return m.astype(np.uint32), pos.astype(np.uint32), d.astype(np.uint8), length


def draw_reads(seed: int):
    rng = np.random.default_rng(seed)
    genomes = [(m, g, rng.integers(0, 2, len(m)).astype(np.uint8)) for m, g in rm.draw_genomes(rng, n_genomes=3, length=1000)]
    cut = lambda gi, start, n: tuple(a[start:start + n] for a in genomes[gi])
    somewhere = lambda n: (lambda gi: cut(gi, int(rng.integers(0, max(1, len(genomes[gi][0]) - 200 - n))), n))(int(rng.integers(0, len(genomes))))
    reads = []
    for _ in range(60):
        reads.append(sample(rng, [somewhere(int(rng.integers(50, 120)))], rng.random() < 0.5, 0.01))
    for _ in range(30):
        reads.append(sample(rng, [somewhere(int(rng.integers(25, 90)))], rng.random() < 0.5, 0.06))
    for _ in range(40):
        reads.append(sample(rng, [somewhere(int(rng.integers(40, 100)))], rng.random() < 0.5, float(rng.uniform(0.10, 0.45)), jitter=1))
    for _ in range(45):                                                  # chimeric: the chain ends inside both reads, a long piece and a short one
        a, b = somewhere(int(rng.integers(80, 130))), somewhere(int(rng.integers(30, 42)))
        reads.append(sample(rng, [a, b] if rng.random() < 0.5 else [b, a], rng.random() < 0.5, 0.01))
    for _ in range(36):                                                  # very noisy reads over one region: identities far below the threshold
        reads.append(sample(rng, [cut(1, int(rng.integers(0, 120)), int(rng.integers(90, 130)))], rng.random() < 0.5, float(rng.uniform(0.28, 0.45)), jitter=1))
    for _ in range(30):
        reads.append(sample(rng, [somewhere(int(rng.integers(2, 14)))], rng.random() < 0.5, 0.01))
    for n in (600, 420, 300):                                            # long reads
        reads.append(sample(rng, [somewhere(n)], rng.random() < 0.5, 0.02))
    rep = len(genomes[0][0]) - 180                                       # where genome 0's long tandem repeat starts (120 minimizers)
    for start, n, rev in ((rep - 30, 110, False), (rep + 20, 130, True), (rep + 60, 110, False), (rep - 10, 70, True)):
        reads.append(sample(rng, [cut(0, start, n)], rev, 0.01, jitter=0))
    for n in (0, 1):
        reads.append(sample(rng, [somewhere(n)], False, 0.0))
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    # the selection: per target up to 8 of the reads that share a minimizer with it, ascending; now and then one that shares none
    owner = {}
    for r, (m, _, _, _) in enumerate(reads):
        for x in set(m.tolist()):
            owner.setdefault(x, []).append(r)
    sel = []
    for t, (m, _, _, _) in enumerate(reads):
        cand = sorted({r for x in set(m.tolist()) for r in owner[x] if r != t})
        if len(cand) > 8:
            cand = sorted(rng.choice(cand, 8, replace=False).tolist())
        if rng.random() < 0.1:
            cand = sorted(set(cand) | {int(rng.integers(0, len(reads)))} - {t})
        sel.append(cand)
    return reads, sel


def run_reference(exe: str, reads, sel, cfg: dict):
    text = [str(len(reads))]
    for m, p, d, length in reads:
        text.append(" ".join([str(len(m)), str(length)] + [f"{int(a)} {int(b)} {int(c)}" for a, b, c in zip(m, p, d)]))
    text.append(str(len(sel)))
    for t, row in enumerate(sel):
        text.append(" ".join([str(t), str(len(row))] + [str(r) for r in row]))
    out = subprocess.run([exe, str(cfg["band"]), str(cfg["max_overhang"]), str(cfg["min_overlap_length"]), repr(cfg["min_identity"]), str(cfg["minimizer_size"])],
                         input=("\n".join(text) + "\n").encode(), capture_output=True, check=True).stdout.decode()
    rows, seconds = [], 0.0
    for line in out.splitlines():
        tag, *f = line.split()
        if tag == "R":
            rows.append([int(x) for x in f])
        elif tag == "T":
            seconds = float(f[0])
    rows = np.array(rows, dtype=np.int64).reshape(-1, len(ROW_FIELDS))
    cat = lambda k, t: np.concatenate([np.asarray(r[k]) for r in reads]).astype(t)
    data = dict(read_offsets=np.concatenate([[0], np.cumsum([len(r[0]) for r in reads])]).astype(np.uint64), minimizers=cat(0, np.uint32), positions=cat(1, np.uint32),
                directions=cat(2, np.uint8), read_lengths=np.array([r[3] for r in reads], np.uint32),
                sel_offsets=np.concatenate([[0], np.cumsum([len(s) for s in sel])]).astype(np.uint64),
                sel_neighbour=np.array([r for s in sel for r in s], np.uint32))
    for c, name in enumerate(ROW_FIELDS):
        if name == "identity_bits":
            data["row_identity"] = rows[:, c].astype(np.uint32).view(np.float32)
        else:
            data["row_" + name] = rows[:, c].astype(np.int32 if name.startswith("n_") and name != "n_anchors" else np.uint8 if name in ("chain", "kept", "query_reversed") else np.uint32)
    assert len(rows) == len(data["sel_neighbour"])
    return data, seconds


def conditions(data: dict, cfg: dict, other_band: dict | None) -> dict:
    """The conditions on the rows (asserted here and again by tests/test_read_verify_model.py): not measurements."""
    chain = data["row_chain"] != 0
    over_s = data["row_overhang_start"] > cfg["max_overhang"]
    over_e = data["row_overhang_end"] > cfg["max_overhang"]
    short = data["row_align_length"] < cfg["min_overlap_length"]
    low = data["row_identity"] < np.float32(cfg["min_identity"])
    fails = over_s.astype(int) + over_e + short + low
    alone = lambda f: int((chain & f & (fails == 1)).sum())
    kept = data["row_kept"] != 0
    assert np.array_equal(kept, chain & (fails == 0))
    reads = vm.fixture_reads(data)
    off = data["read_offsets"].astype(np.int64)
    multi = 0
    so = data["sel_offsets"].astype(np.int64)
    for t in range(len(so) - 1):
        tm = data["minimizers"][off[t]:off[t + 1]]
        for s in range(so[t], so[t + 1]):
            q = int(data["sel_neighbour"][s])
            qm = data["minimizers"][off[q]:off[q + 1]]
            vals, counts = np.unique(qm, return_counts=True)
            multi += bool(np.isin(tm, vals[counts > 1]).any())
    table = vm.min_matches(int(np.diff(off).max()), cfg["min_identity"], cfg["minimizer_size"])
    m, mis = data["row_n_matches"].astype(np.int64), data["row_n_mismatches"].astype(np.int64)
    seeds = np.minimum(m + mis + data["row_n_deletions"], m + mis + data["row_n_insertions"])
    c = dict(rows=len(chain), chains=int(chain.sum()), rejected_by_start_overhang_alone=alone(over_s), rejected_by_end_overhang_alone=alone(over_e),
             rejected_by_length_alone=alone(short), rejected_by_identity_alone=alone(low), kept=int(kept.sum()), kept_reversed=int((kept & (data["row_query_reversed"] != 0)).sum()),
             rows_3_anchors_up_without_chain=int(((data["row_n_anchors"] >= 3) & ~chain).sum()), rows_below_3_anchors=int((data["row_n_anchors"] < 3).sum()),
             rows_with_a_minimizer_meeting_several=int(multi), rows_at_min_matches=int((chain & (m == table[seeds])).sum()),
             rows_one_below_min_matches=int((chain & (m + 1 == table[seeds])).sum()))
    for k in ("rejected_by_start_overhang_alone", "rejected_by_end_overhang_alone", "rejected_by_length_alone", "rejected_by_identity_alone"):
        assert c[k] >= 20, c
    assert c["kept"] >= 50 and c["kept_reversed"] >= 15, c
    assert c["rows_3_anchors_up_without_chain"] >= 10 and c["rows_below_3_anchors"] >= 10 and c["rows_with_a_minimizer_meeting_several"] >= 10, c
    assert c["rows_at_min_matches"] >= 5 and c["rows_one_below_min_matches"] >= 5, c
    if other_band is not None:
        differ = np.zeros(len(chain), bool)
        for k in ("chain",) + vm.SUMMARY_FIELDS:
            differ |= data["row_" + k] != other_band["row_" + k]
        c["rows_changed_between_band_5_and_62"] = int(differ.sum())
        assert c["rows_changed_between_band_5_and_62"] >= 5, c
    # ... and the numpy model equals the reference on the whole fixture:
    vm.same(vm.verify(data["sel_offsets"], data["sel_neighbour"], reads, **vm.fixture_params(cfg)), vm.fixture_verification(data))
    return c


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's checkout (holds src/Commons.hpp)")
    ap.add_argument("--first-seed", type=int, default=8100)
    args = ap.parse_args()
    manifest = dict(delta_coded=list(DELTA_CODED), configs=[])
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "verify_ref")
        subprocess.run(["g++", "-std=gnu++20", "-O2", "-w", "-fopenmp", "-I" + os.path.join(args.ref, "src"), "-I" + args.ref,
                        os.path.join(HERE, "verify_ref.cpp"), os.path.join(args.ref, "src", "utils", "MurmurHash3.cpp"), "-lz", "-o", exe], check=True)
        seed = args.first_seed
        for cfg in CONFIGS:
            while True:
                reads, sel = draw_reads(seed)
                data, seconds = run_reference(exe, reads, sel, cfg)
                other = None
                if cfg["band"] in (5, 62):
                    other, _ = run_reference(exe, reads, sel, dict(cfg, band=67 - cfg["band"]))
                try:
                    found = conditions(data, cfg, other)
                    break
                except AssertionError as e:
                    print(cfg["name"], "seed", seed, "does not meet the conditions:", e)
                    seed += 1
            path = os.path.join(HERE, cfg["name"] + ".npz")
            np.savez_compressed(path, **{k: (np.diff(v.astype(np.int64), prepend=0).astype(np.int32) if k in DELTA_CODED else v) for k, v in data.items()})
            assert os.path.getsize(path) <= SIZE_LIMIT, (os.path.getsize(path), SIZE_LIMIT)
            manifest["configs"].append(dict(cfg, seed=seed, n_reads=len(reads), n_minimizers=int(data["read_offsets"][-1]), n_targets=len(sel),
                                            n_anchors=int(data["row_n_anchors"].sum()), reference_seconds=round(seconds, 4), **found))
            print(cfg["name"], "seed", seed, os.path.getsize(path), "bytes of fixture", manifest["configs"][-1])
            seed += 1
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
