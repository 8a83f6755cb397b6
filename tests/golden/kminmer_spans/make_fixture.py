"""Regenerates tests/golden/kminmer_spans: the reads (seeded) and, per configuration, what the REFERENCE computes for them --
EncoderRLE::execute, MinimizerParser::parse and MDBG::getKminmers, called by spans_ref.cpp, which is compiled here against the
reference's sources with the flags of oracle/Makefile.  No test runs this; only the data it wrote is read by tests/test_gpu_kminmer_spans.py.

    python tests/golden/kminmer_spans/make_fixture.py --ref <path of the reference>

Files: reads.txt (one read a line), manifest.json (the configurations), <name>.npz (the reference's answers of one configuration:
offsets / minimizers / pos / min_start / min_end per minimizer, window_offsets, and per window reversed, hash_hi, hash_lo, pos_start,
pos_end, length, seq_length_start, seq_length_end).  The four _position_of_* fields are checked to be 0 and not stored.

The configuration without homopolymer compression keeps the end trim: with trim 0 the reference reads one element behind its
rlePositions when a read's last l-mer is selected (spans_ref stops if that is asked for)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# name, l, density, hpc, trim (MinimizerParser::_trimBps), k, longest read taken (0 = all), valid_only: only reads without a character that
# has bit 3 set (N, n, K, M, Y ...).  An l-mer over such a character is invalid: the reference gives it the value -1 "to be skipped as a
# minimizer" (utils/kmer/Kmer.hpp:567, :580), which holds at every density of practice and not at 1.0, where -1 hashes below the bound and is
# selected; mdbg_scan never selects an invalid l-mer.  The configuration that selects every position therefore takes reads made of A, C, G, T
# in either case.
CONFIGS = [
    dict(name="l15_hpc_k4", l=15, density=0.05, hpc=1, trim=1, k=4, max_len=0, valid_only=0),
    dict(name="l15_hpc_k13", l=15, density=0.1, hpc=1, trim=1, k=13, max_len=0, valid_only=0),
    # every position selected and no end trim: the read's last l-mer is a minimizer and its end is the sentinel rle[L']
    dict(name="l13_hpc_all_k2", l=13, density=1.0, hpc=1, trim=0, k=2, max_len=1000, valid_only=1),
    dict(name="l15_plain_k5", l=15, density=0.05, hpc=0, trim=1, k=5, max_len=0, valid_only=0),
]


def make_reads(seed: int = 2024) -> list[bytes]:
    rng = np.random.default_rng(seed)

    def read(n: int, letters: bytes, long_run: int) -> bytes:
        out = bytearray()
        while len(out) < n:
            c = letters[int(rng.integers(0, len(letters)))]
            d = int(rng.integers(0, 1000))
            run = 1 if d < 650 else int(rng.integers(2, 6)) if d < 960 else int(rng.integers(6, 30)) if d < 995 else int(rng.integers(30, long_run + 1))
            out += bytes([c]) * run
        return bytes(out[:n])

    plain, soft, iupac = b"ACGT", b"ACGTacgt", b"ACGTNNRYKMSWacgtn"
    reads = [read(n, plain, 90) for n in (1, 12, 13, 14, 15, 16, 17, 30, 31, 32, 33, 63, 64, 65, 100, 250, 400, 700, 1000)]
    reads += [read(int(rng.integers(100, 3000)), plain, 90) for _ in range(12)]
    reads += [read(int(rng.integers(40, 2500)), soft, 40) for _ in range(5)]
    reads += [read(int(rng.integers(40, 2500)), iupac, 40) for _ in range(5)]
    reads += [b"ACGTTGCA" * 20 + b"N" * 37 + read(300, plain, 40) + b"GNGNNG" + read(200, plain, 40), b"aA" * 30 + read(500, plain, 40) + b"AaAaaA"]
    reads.insert(20, read(70_000, plain, 90))                 # the one long line
    return reads


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's checkout (holds src/Commons.hpp)")
    args = ap.parse_args()
    reads = make_reads()
    with open(os.path.join(HERE, "reads.txt"), "wb") as f:
        f.write(b"".join(r + b"\n" for r in reads))
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "spans_ref")
        subprocess.run(["g++", "-std=gnu++20", "-O2", "-w", "-fopenmp", "-I" + os.path.join(args.ref, "src"), "-I" + args.ref,
                        os.path.join(HERE, "spans_ref.cpp"), os.path.join(args.ref, "src", "utils", "MurmurHash3.cpp"), "-lz", "-o", exe], check=True)
        manifest = dict(reads="reads.txt", n_reads=len(reads), configs=[])
        for cfg in CONFIGS:
            take = [i for i, r in enumerate(reads) if (not cfg["max_len"] or len(r) <= cfg["max_len"]) and not (cfg["valid_only"] and any(c & 8 for c in r))]
            text = b"".join(reads[i] + b"\n" for i in take)
            out = subprocess.run([exe, str(cfg["l"]), repr(cfg["density"]), str(cfg["hpc"]), str(cfg["trim"]), str(cfg["k"])], input=text,
                                 capture_output=True, check=True).stdout.decode()
            n_min = np.zeros(len(take), np.uint64)
            n_win = np.zeros(len(take), np.uint64)
            M, W = [], []
            for line in out.splitlines():
                t = line.split()
                if t[0] == "R":
                    n_min[int(t[1])], n_win[int(t[1])] = int(t[2]), int(t[3])
                elif t[0] == "M":
                    M.append([int(x) for x in t[2:]])
                else:
                    W.append([int(x) for x in t[2:]])
            M = np.array(M, dtype=np.uint64).reshape(-1, 4)
            W = np.array(W, dtype=np.uint64).reshape(-1, 12)
            assert len(M) == n_min.sum() and len(W) == n_win.sum()
            assert not W[:, 8:].any(), "the four _position_of_* fields are 0 in the reference"
            assert np.array_equal(W[:, 5], W[:, 4] - W[:, 3]), "_length is pos_end - pos_start"
            np.savez_compressed(
                os.path.join(HERE, cfg["name"] + ".npz"),
                offsets=np.concatenate([[0], np.cumsum(n_min)]).astype(np.uint64), minimizers=M[:, 0].astype(np.uint32), pos=M[:, 1].astype(np.uint32),
                min_start=M[:, 2].astype(np.uint32), min_end=M[:, 3].astype(np.uint32),
                window_offsets=np.concatenate([[0], np.cumsum(n_win)]).astype(np.uint64), reversed=W[:, 0].astype(np.uint8), hash_hi=W[:, 1], hash_lo=W[:, 2],
                pos_start=W[:, 3].astype(np.uint32), pos_end=W[:, 4].astype(np.uint32), length=W[:, 5].astype(np.uint32),
                seq_length_start=W[:, 6].astype(np.uint32), seq_length_end=W[:, 7].astype(np.uint32))
            manifest["configs"].append(dict(cfg, reads=take, n_minimizers=int(len(M)), n_windows=int(len(W)), n_reversed=int(W[:, 0].sum())))
            print(cfg["name"], len(take), "reads", len(M), "minimizers", len(W), "windows", int(W[:, 0].sum()), "reversed")
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
