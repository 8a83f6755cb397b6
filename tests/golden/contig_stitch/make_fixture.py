"""Regenerates tests/golden/contig_stitch: per configuration seeded contigs and the text the REFERENCE writes for them --
ToBasespaceGfa::CreateBaseContigsFunctor::operator() over pieces stored as DnaBitset2(extractKminmerSequence(...)), called by
contigs_ref.cpp, which is compiled here against the reference's sources with the flags of oracle/Makefile.  No test runs this; only the
data it wrote is read by tests/test_contig_stitch_model.py and tests/test_gpu_contig_stitch.py.

    python tests/golden/contig_stitch/make_fixture.py --ref <path of the reference>

The reads are tests/golden/kminmer_sequences/reads.txt and the configurations two of its manifest's: l15_hpc_k4 (homopolymer compression)
and l15_plain_k5 (none); both include the reads with islands of N, K, M, Y.  Reads the library and DnaBitset2 cannot agree on (lower case,
R / S / W) are left out exactly as that fixture leaves them out -- the configuration's `reads` list is taken as it stands -- and
manifest.json records the count; nothing else is dropped.

A contig is a seeded random list of (read, window of the read, contig window reversed, present): the functor does not care whether
neighbouring pieces overlap coherently, so arbitrary picks test more.  Within a contig no (read, window) repeats (the reference's maps hold
one piece per read position and type).  A piece that is not present is left out of the reference's map: "no sequence for this k-min-mer".

Files: manifest.json, <name>.npz -- contig_offsets (n + 1), per position read (index into the configuration's reads), window, reversed,
present; per contig names and flags; text: the inflated bytes the functor wrote through gzwrite."""
from __future__ import annotations

import argparse
import gzip
import json
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEQUENCES = os.path.join(os.path.dirname(HERE), "kminmer_sequences")
SPANS = os.path.join(os.path.dirname(HERE), "kminmer_spans")
CONFIGS = ("l15_hpc_k4", "l15_plain_k5")
NAMES_FIRST = (0, 4294967295, 7, 42, 1000000000, 99, 9)


def draw_contigs(rng, reads: list[bytes], n_win: np.ndarray) -> tuple[list, np.ndarray, np.ndarray]:
    woff = np.concatenate([[0], np.cumsum(n_win)])
    flat_read = np.repeat(np.arange(len(n_win)), n_win)
    with_bit3 = np.flatnonzero([any(c & 8 for c in reads[r]) for r in flat_read])

    def contig(pool, n, p_present=0.9):
        picks = rng.choice(pool, size=min(n, len(pool)), replace=False)
        return [(int(flat_read[w]), int(w - woff[flat_read[w]]), int(rng.integers(0, 2)), int(rng.random() < p_present)) for w in picks]

    everything = np.arange(int(woff[-1]))
    contigs = [contig(everything, int(min(1 + rng.geometric(0.2), 14))) for _ in range(330)]
    contigs += [contig(with_bit3, int(rng.integers(1, 6)), 1.0) for _ in range(40)]           # pieces that cover a bit-3 character, either flip
    first_missing = contig(everything, 5, 1.0)
    first_missing[0] = first_missing[0][:3] + (0,)
    contigs += [first_missing, [p[:3] + (0,) for p in contig(everything, 4)], [], contig(everything, 1, 1.0), []]
    order = rng.permutation(len(contigs))
    contigs = [contigs[i] for i in order]
    names = np.array(list(NAMES_FIRST) + [int(rng.integers(0, 10 ** int(rng.integers(1, 10)))) for _ in range(len(contigs) - len(NAMES_FIRST))], dtype=np.uint32)
    flags = rng.integers(0, 3, len(contigs)).astype(np.uint8)
    return contigs, names, flags


def conditions(reads: list[bytes], spans, contigs, names, flags) -> dict:
    """The conditions on the selection (asserted here and again by tests/test_contig_stitch_model.py): not measurements."""
    woff = spans["window_offsets"].astype(np.int64)
    combos = np.zeros((2, 2, 2), np.int64)
    residues, bit3 = set(), [0, 0]
    first_missing = all_missing = empty = 0
    for contig in contigs:
        at = 0
        empty += not contig
        all_missing += bool(contig) and not any(p[3] for p in contig)
        first_missing += bool(contig) and not contig[0][3] and any(p[3] for p in contig)
        for i, (read, window, rev, present) in enumerate(contig):
            if not present:
                continue
            w = int(woff[read]) + window
            wrev, ps, pe, ls, le = (int(spans[f][w]) for f in ("reversed", "pos_start", "pos_end", "seq_length_start", "seq_length_end"))
            combos[int(i > 0), wrev, rev] += 1
            part = 0 if i == 0 else 1 if rev else 2
            start = ps if part == 0 else ((pe - ls if wrev else ps) if part == 1 else (ps if wrev else pe - le))
            length = pe - ps if part == 0 else ls if part == 1 else le
            if length:
                residues.add(at % 32)
            bit3[rev] += any(c & 8 for c in reads[read][start:start + length])
            at += length
    assert combos.min() >= 50, combos
    assert residues == set(range(32)), sorted(residues)
    assert bit3[0] >= 1 and bit3[1] >= 1, bit3
    assert first_missing >= 1 and all_missing >= 1 and empty >= 1
    assert set(int(f) for f in flags) == {0, 1, 2}
    widths = {len(str(int(n))) for n in names}
    assert {1, 2, 10} <= widths and 0 in names and 4294967295 in names
    return dict(combos=[int(x) for x in combos.ravel()], cover_bit3_unflipped=int(bit3[0]), cover_bit3_flipped=int(bit3[1]), first_missing=int(first_missing),
                all_missing=int(all_missing), no_window=int(empty))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's checkout (holds src/Commons.hpp)")
    args = ap.parse_args()
    with open(os.path.join(SEQUENCES, "reads.txt"), "rb") as f:
        all_reads = f.read().split(b"\n")[:-1]
    with open(os.path.join(SEQUENCES, "manifest.json")) as f:
        configs = {c["name"]: c for c in json.load(f)["configs"]}
    manifest = dict(reads=os.path.join("..", "kminmer_sequences", "reads.txt"), spans="../kminmer_sequences/<name>.npz", configs=[])
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "contigs_ref")
        subprocess.run(["g++", "-std=gnu++20", "-O2", "-w", "-fopenmp", "-I" + os.path.join(args.ref, "src"), "-I" + args.ref,
                        os.path.join(HERE, "contigs_ref.cpp"), os.path.join(args.ref, "src", "utils", "MurmurHash3.cpp"), "-lz", "-o", exe], check=True)
        for seed, name in enumerate(CONFIGS):
            cfg = configs[name]
            reads = [all_reads[i] for i in cfg["reads"]]
            spans = np.load(os.path.join(SEQUENCES, name + ".npz"))
            n_win = np.diff(spans["window_offsets"].astype(np.int64))
            contigs, names, flags = draw_contigs(np.random.default_rng(4100 + seed), reads, n_win)
            found = conditions(reads, spans, contigs, names, flags)
            listing = os.path.join(tmp, name + ".contigs")
            with open(listing, "w") as f:
                for contig, nm, fl in zip(contigs, names, flags):
                    f.write(f"C {int(nm)} {int(fl)} {len(contig)}\n" + "".join("%d %d %d %d\n" % p for p in contig))
            gz = os.path.join(tmp, name + ".fasta.gz")
            out = subprocess.run([exe, str(cfg["l"]), repr(cfg["density"]), str(cfg["hpc"]), str(cfg["trim"]), str(cfg["k"]), listing, gz],
                                 input=b"".join(r + b"\n" for r in reads), capture_output=True, check=True).stdout.decode()
            counted = np.array([int(line.split()[2]) for line in out.splitlines() if line.startswith("R ")])
            assert np.array_equal(counted, n_win), "the driver's windows are not those of tests/golden/kminmer_sequences"
            with gzip.open(gz, "rb") as f:
                text = f.read()
            assert text.count(b">ctg") == len(contigs)
            flat = [p for c in contigs for p in c]
            cols = np.array(flat, dtype=np.int64).reshape(-1, 4)
            path = os.path.join(HERE, name + ".npz")
            np.savez_compressed(path, contig_offsets=np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.uint64), read=cols[:, 0].astype(np.uint32),
                                window=cols[:, 1].astype(np.uint32), reversed=cols[:, 2].astype(np.uint8), present=cols[:, 3].astype(np.uint8), names=names,
                                flags=flags, text=np.frombuffer(text, dtype=np.uint8))
            limit = max(os.path.getsize(os.path.join(SPANS, f)) for f in os.listdir(SPANS))
            assert os.path.getsize(path) <= limit, (os.path.getsize(path), limit)
            manifest["configs"].append(dict({f: cfg[f] for f in ("name", "l", "density", "hpc", "trim", "k", "reads", "left_out")}, n_contigs=len(contigs),
                                            n_positions=len(flat), n_text_bytes=len(text), **found))
            print(name, len(contigs), "contigs", len(flat), "positions", len(text), "bytes of text", os.path.getsize(path), "bytes of fixture", found)
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
