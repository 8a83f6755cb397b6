"""Regenerates tests/golden/read_realign: the reads of tests/golden/read_verify's generator with a quality byte per minimizer, the kept
(target, neighbour) rows and flags the REFERENCE's verify step gives for them -- every fourth kept row's flag flipped on purpose, so that the
reversed form of the alignment list is there at all -- and what the reference's Utils::getLowDensityMinimizerRead, Utils::isReadTooShort,
MinimizerRead::toReverseComplement and MinimizerChainer::computeChainingAlignment (normalizeAlignment included) leave of every kept row at
assembly density -- by realign_ref.cpp, compiled here against the reference's sources exactly as tests/golden/read_verify/make_fixture.py
compiles its driver.  No test runs this; only the data it wrote is read by tests/test_read_realign_model.py and tests/test_gpu_read_realign.py.

    python tests/golden/read_realign/make_fixture.py --ref <path of the reference>

Configurations: (band 62, density 0.2), (band 5, density 0.2), (band 62, density 0.5); the verify step's other thresholds are read_verify's
band62 (1000, 1000, 0.96f, 15), min_minimizers 10.  The densities are far above the reference's 0.005: the reads are 0 - 600 minimizers long,
and what matters is the ratio to the correction density, 0.2 in the reference's defaults (0.005 / 0.025).  The conditions on the rows are
asserted below (conditions, not measurements; manifest.json records the counts) -- seeds are tried in order until the reference's output
meets them.

Files: manifest.json, <name>.npz --
  qualities                                                   one byte per minimizer of the reads
  read_offsets, minimizers, positions, directions, read_lengths      the reads -- left out when a read_verify file holds the very same
                                                              (manifest: reads_from), as it does for the seed read_verify's band62 took
  thin_index                                                  the minimizers (flat indexes) the reference's thinning keeps
  kept_offsets (targets + 1; target t is read t), kept_neighbour, kept_reversed (the flag GIVEN), kept_flipped
  row_state (0 no chain, 1 chain, 16 short), row_<field>, row_query_checksum      per kept row what the reference computed
  entry_ref_index, entry_query_index (0xFFFFFFFF none), entry_kind, entry_query_quality      the lists after normalizeAlignment
The arrays manifest.json lists under delta_coded are stored as first differences (tests/realign_model.py, load_fixture, sums them up)."""
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
from tests import realign_model as rm  # noqa: E402
from tests import verify_model as vm  # noqa: E402

_spec = importlib.util.spec_from_file_location("read_verify_fixture", os.path.join(os.path.dirname(HERE), "read_verify", "make_fixture.py"))
rv = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rv)

VERIFY = dict(max_overhang=1000, min_overlap_length=1000, min_identity=0.96, minimizer_size=15)
CONFIGS = (dict(name="band62_d20", band=62, density=0.2, min_minimizers=10), dict(name="band5_d20", band=5, density=0.2, min_minimizers=10),
           dict(name="band62_d50", band=62, density=0.5, min_minimizers=10))
FLIP_EVERY = 4
DELTA_CODED = ("positions", "thin_index", "kept_neighbour", "entry_ref_index", "entry_query_index")
ROW_FIELDS = ("state", "n_anchors", "chain_reversed", "n_matches", "n_mismatches", "n_deletions", "n_insertions", "reference_start_index", "reference_end_index", "n_entries",
              "query_checksum")
READ_ARRAYS = ("read_offsets", "minimizers", "positions", "directions", "read_lengths")
SIZE_LIMIT = rv.SIZE_LIMIT          # the precedent: 128 918 bytes


def draw_qualities(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed + 1_000_000).integers(0, 41, n).astype(np.uint8)


def run_reference(exe: str, reads, sel, qual, cfg: dict):
    off = np.concatenate([[0], np.cumsum([len(r[0]) for r in reads])]).astype(np.int64)
    text = [str(len(reads))]
    for r, (m, p, d, length) in enumerate(reads):
        q = qual[off[r]:off[r + 1]]
        text.append(" ".join([str(len(m)), str(length)] + [f"{int(a)} {int(b)} {int(c)} {int(e)}" for a, b, c, e in zip(m, p, d, q)]))
    text.append(str(len(sel)))
    for t, row in enumerate(sel):
        text.append(" ".join([str(t), str(len(row))] + [str(r) for r in row]))
    out = subprocess.run([exe, str(cfg["band"]), str(VERIFY["max_overhang"]), str(VERIFY["min_overlap_length"]), repr(VERIFY["min_identity"]), str(VERIFY["minimizer_size"]),
                          repr(cfg["density"]), str(FLIP_EVERY)], input=("\n".join(text) + "\n").encode(), capture_output=True, check=True).stdout.decode()
    thin, kept, rows, entries, seconds = [], [[] for _ in sel], [], [], 0.0
    for line in out.splitlines():
        tag, *f = line.split()
        if tag == "D":
            assert int(f[1]) == len(f) - 2
            thin += [int(off[int(f[0])]) + int(x) for x in f[2:]]
        elif tag == "K":
            v = [int(x) for x in f]
            kept[v[0]].append(v[1:4])
            rows.append(v[4:15])
            assert len(v) == 15 + 4 * v[13], line[:80]
            entries += v[15:]
        elif tag == "T":
            seconds = float(f[0])
    rows = np.array(rows, np.int64).reshape(-1, len(ROW_FIELDS))
    entries = np.array(entries, np.int64).reshape(-1, 4)
    cat = lambda k, t: np.concatenate([np.asarray(r[k]) for r in reads]).astype(t)
    flat = [x for k in kept for x in k]
    data = dict(read_offsets=off.astype(np.uint64), minimizers=cat(0, np.uint32), positions=cat(1, np.uint32), directions=cat(2, np.uint8),
                read_lengths=np.array([r[3] for r in reads], np.uint32), qualities=qual, thin_index=np.array(thin, np.uint32),
                kept_offsets=np.concatenate([[0], np.cumsum([len(k) for k in kept])]).astype(np.uint64), kept_neighbour=np.array([x[0] for x in flat], np.uint32),
                kept_reversed=np.array([x[1] for x in flat], np.uint8), kept_flipped=np.array([x[2] for x in flat], np.uint8),
                entry_ref_index=(entries[:, 0] & 0xFFFFFFFF).astype(np.uint32), entry_query_index=(entries[:, 1] & 0xFFFFFFFF).astype(np.uint32),
                entry_kind=entries[:, 2].astype(np.uint8), entry_query_quality=entries[:, 3].astype(np.uint8))
    for c, name in enumerate(ROW_FIELDS):
        data["row_" + name] = rows[:, c].astype(np.int32 if name in ("n_matches", "n_mismatches", "n_deletions", "n_insertions") else np.uint8 if name in ("state", "chain_reversed") else np.uint32)
    assert len(rows) == len(flat) and len(entries) == int(rows[:, 9].sum())
    return data, seconds


def conditions(data: dict, cfg: dict) -> dict:
    """The conditions on the rows (asserted here and again by tests/test_read_realign_model.py): not measurements."""
    state = data["row_state"]
    chain = state == rm.REALIGN_CHAIN
    eo = np.concatenate([[0], np.cumsum(data["row_n_entries"].astype(np.int64))])
    matches_after = np.array([int((data["entry_kind"][eo[s]:eo[s + 1]] == rm.MATCH).sum()) for s in range(len(state))])
    off, ko = data["read_offsets"].astype(np.int64), data["kept_offsets"].astype(np.int64)
    keep = np.zeros(int(off[-1]), bool)
    keep[data["thin_index"]] = True
    thin = lambda r: data["minimizers"][off[r]:off[r + 1]][keep[off[r]:off[r + 1]]]
    target = np.repeat(np.arange(len(ko) - 1), np.diff(ko))
    multi = 0                                          # rows in which a neighbour minimizer meets several target minimizers
    for t, q, st in zip(target, data["kept_neighbour"], state):
        if st == rm.REALIGN_SHORT:
            continue
        vals, counts = np.unique(thin(t), return_counts=True)
        multi += bool(np.isin(thin(int(q)), vals[counts > 1]).any())
    c = dict(kept_rows=len(state), flipped_rows=int(data["kept_flipped"].sum()), short_rows=int((state == rm.REALIGN_SHORT).sum()), rows_without_chain=int((state == 0).sum()),
             chains=int(chain.sum()), reversed_chains=int((chain & (data["row_chain_reversed"] != 0)).sum()),
             reversed_chains_unflipped=int((chain & (data["row_chain_reversed"] != 0) & (data["kept_flipped"] == 0)).sum()),
             rows_where_normalisation_made_a_match=int((chain & (matches_after > data["row_n_matches"])).sum()), longest_list=int(data["row_n_entries"].max()),
             lists_above_64_entries=int((data["row_n_entries"] > 64).sum()), n_entries=int(eo[-1]), rows_with_a_minimizer_meeting_several=int(multi))
    if cfg["density"] == 0.2:
        assert c["short_rows"] >= 50 and c["rows_without_chain"] >= 40 and c["chains"] >= 300 and c["reversed_chains"] >= 50, c
        assert c["rows_where_normalisation_made_a_match"] >= 10, c
    if cfg["density"] == 0.5:
        assert c["lists_above_64_entries"] >= 1, c
    assert c["rows_with_a_minimizer_meeting_several"] >= 10, c
    # ... and the numpy model equals the reference on the whole fixture:
    got = rm.realign(data["kept_offsets"], data["kept_neighbour"], data["kept_reversed"], vm.fixture_reads(data), data["qualities"], **rm.fixture_params(cfg))
    rm.same_as_fixture(got, rm.fixture_realignment(data))
    return c


def reads_from(data: dict) -> str | None:
    """the read_verify file that holds these very reads, if any"""
    for name in (c["name"] for c in vm.fixture_manifest()["configs"]):
        v = vm.load_fixture(name)
        if all(v[k].shape == data[k].shape and np.array_equal(v[k], data[k]) for k in READ_ARRAYS):
            return name
    return None


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's checkout (holds src/Commons.hpp)")
    ap.add_argument("--first-seed", type=int, default=8100)
    args = ap.parse_args()
    manifest = dict(delta_coded=list(DELTA_CODED), flip_every=FLIP_EVERY, verify=VERIFY, configs=[])
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "realign_ref")
        subprocess.run(["g++", "-std=gnu++20", "-O2", "-w", "-fopenmp", "-I" + os.path.join(args.ref, "src"), "-I" + args.ref,
                        os.path.join(HERE, "realign_ref.cpp"), os.path.join(args.ref, "src", "utils", "MurmurHash3.cpp"), "-lz", "-o", exe], check=True)
        for cfg in CONFIGS:
            seed = args.first_seed
            while True:
                reads, sel = rv.draw_reads(seed)
                qual = draw_qualities(seed, sum(len(r[0]) for r in reads))
                data, seconds = run_reference(exe, reads, sel, qual, cfg)
                try:
                    found = conditions(data, cfg)
                    break
                except AssertionError as e:
                    print(cfg["name"], "seed", seed, "does not meet the conditions:", e)
                    seed += 1
            source = reads_from(data)
            stored = {k: v for k, v in data.items() if not (source and k in READ_ARRAYS)}
            path = os.path.join(HERE, cfg["name"] + ".npz")
            np.savez_compressed(path, **{k: (np.diff(v.astype(np.int64), prepend=0).astype(np.int32) if k in DELTA_CODED else v) for k, v in stored.items()})
            assert os.path.getsize(path) <= SIZE_LIMIT, (os.path.getsize(path), SIZE_LIMIT)
            manifest["configs"].append(dict(cfg, seed=seed, reads_from=source, n_reads=len(reads), n_minimizers=int(data["read_offsets"][-1]),
                                            n_thinned=len(data["thin_index"]), n_targets=len(sel), n_anchors=int(data["row_n_anchors"].sum()),
                                            reference_seconds=round(seconds, 4), **found))
            print(cfg["name"], "seed", seed, os.path.getsize(path), "bytes of fixture", manifest["configs"][-1])
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
