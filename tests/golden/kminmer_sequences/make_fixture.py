"""Regenerates tests/golden/kminmer_sequences: the reads and, per configuration, what the REFERENCE cuts out of them --
ToBasespaceGfa::extractKminmerSequence over the windows of MDBG::getKminmers, packed by DnaBitset2, called by sequences_ref.cpp, which is
compiled here against the reference's sources with the flags of oracle/Makefile.  No test runs this; only the data it wrote is read by
tests/test_kminmer_sequences_model.py and tests/test_gpu_kminmer_sequences.py.

    python tests/golden/kminmer_sequences/make_fixture.py --ref <path of the reference>

The reads are those of tests/golden/kminmer_spans (its generator's make_reads, the same indices) followed by reads that put islands of
N, K, M, Y between clean stretches, so that windows span one.  The configurations are the four of kminmer_spans/manifest.json.

Reads with a lower-case letter or an IUPAC letter without bit 3 (R, S, W) are LEFT OUT of a configuration: the packed reads keep no case,
so the library returns the base the 2-bit code names where DnaBitset2 stores A (include/mdbg_hip.h says so); tests/extract_model.py
covers them.  manifest.json records how many were left out, and nothing else may be.

Requests: every window x Entire / Left / Right of the reads of at most 3000 bases, every 16th window of the 70 kb read.

Files: reads.txt (one read a line), manifest.json, <name>.npz -- per window of the configuration's reads window_offsets, reversed, pos_start,
pos_end, seq_length_start, seq_length_end (ReadKminmer's fields); per request req_window (flat index), req_part, lengths (bases) and, in
`bitset`, DnaBitset2::_m_data of every request back to back (ceil(length / 4) bytes each)."""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SPANS = os.path.join(os.path.dirname(HERE), "kminmer_spans")
ALL_UPTO, STRIDE = 3000, 16
PLAIN = set(b"ACGT")


def spans_reads() -> list[bytes]:
    spec = importlib.util.spec_from_file_location("spans_make_fixture", os.path.join(SPANS, "make_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    reads = mod.make_reads()
    with open(os.path.join(SPANS, "reads.txt"), "rb") as f:
        assert f.read().split(b"\n")[:-1] == reads, "tests/golden/kminmer_spans/reads.txt is not what its generator makes"
    return reads


def island_reads(seed: int = 2025) -> list[bytes]:
    rng = np.random.default_rng(seed)

    def clean(n: int) -> bytes:
        out = bytearray()
        while len(out) < n:
            out += bytes([b"ACGT"[int(rng.integers(0, 4))]]) * (1 if rng.integers(0, 10) < 7 else int(rng.integers(2, 6)))
        return bytes(out[:n])

    return [clean(500) + b"N" + clean(500),
            clean(400) + b"NN" + clean(400) + b"NNNNN" + clean(400),
            clean(300) + b"K" + clean(300) + b"MMM" + clean(300) + b"Y" + clean(300),
            clean(600) + b"N" * 20 + clean(600),
            clean(77) + b"N" + clean(150) + b"N" + clean(33) + b"NNN" + clean(240)]


def comparable(r: bytes) -> bool:
    """Every character is A, C, G, T or has bit 3 set: the library and DnaBitset2 agree on it."""
    return all(c in PLAIN or c & 8 for c in r)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's checkout (holds src/Commons.hpp)")
    args = ap.parse_args()
    base = spans_reads()
    reads = base + island_reads()
    soft_or_iupac = sum(not comparable(r) for r in base)
    with open(os.path.join(HERE, "reads.txt"), "wb") as f:
        f.write(b"".join(r + b"\n" for r in reads))
    with open(os.path.join(SPANS, "manifest.json")) as f:
        configs = json.load(f)["configs"]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sequences_ref")
        subprocess.run(["g++", "-std=gnu++20", "-O2", "-w", "-fopenmp", "-I" + os.path.join(args.ref, "src"), "-I" + args.ref,
                        os.path.join(HERE, "sequences_ref.cpp"), os.path.join(args.ref, "src", "utils", "MurmurHash3.cpp"), "-lz", "-o", exe], check=True)
        manifest = dict(reads="reads.txt", n_reads=len(reads), n_spans_reads=len(base), all_upto=ALL_UPTO, stride=STRIDE, configs=[])
        for spans_cfg in configs:
            cfg = {f: spans_cfg[f] for f in ("name", "l", "density", "hpc", "trim", "k", "max_len", "valid_only")}
            fits = lambda r: (not cfg["max_len"] or len(r) <= cfg["max_len"]) and not (cfg["valid_only"] and any(c & 8 for c in r))
            take = [i for i in spans_cfg["reads"] if comparable(reads[i])] + [i for i in range(len(base), len(reads)) if fits(reads[i])]
            left_out = len(spans_cfg["reads"]) - sum(comparable(reads[i]) for i in spans_cfg["reads"])
            assert left_out <= soft_or_iupac and all(not comparable(reads[i]) for i in spans_cfg["reads"] if i not in take)
            text = b"".join(reads[i] + b"\n" for i in take)
            out = subprocess.run([exe, str(cfg["l"]), repr(cfg["density"]), str(cfg["hpc"]), str(cfg["trim"]), str(cfg["k"]), str(ALL_UPTO), str(STRIDE)],
                                 input=text, capture_output=True, check=True).stdout.decode()
            n_win = np.zeros(len(take), np.int64)
            W, Q, lengths, blobs = [], [], [], []
            for line in out.splitlines():
                t = line.split()
                if t[0] == "R":
                    n_win[int(t[1])] = int(t[3])
                elif t[0] == "W":
                    W.append([int(x) for x in t[1:]])
                else:
                    Q.append([int(x) for x in t[1:4]])
                    lengths.append(int(t[4]))
                    blobs.append(b"" if t[5] == "-" else bytes.fromhex(t[5]))
            W = np.array(W, dtype=np.int64).reshape(-1, 6)
            Q = np.array(Q, dtype=np.int64).reshape(-1, 3)
            lengths = np.array(lengths, dtype=np.int64)
            woff = np.concatenate([[0], np.cumsum(n_win)])
            assert len(W) == woff[-1] and all(len(b) == (n + 3) // 4 for b, n in zip(blobs, lengths))
            flat = woff[Q[:, 0]] + Q[:, 1]
            part = Q[:, 2]
            rev, ps, pe, ls, le = (W[flat, c] for c in (1, 2, 3, 4, 5))
            # ---- conditions on the selection (not measurements) -------------------------------------------------------------------------
            # the range of the read a request covers, by the three-part rule the header states
            start = np.where(part == 0, ps, np.where(part == 1, np.where(rev == 1, pe - ls, ps), np.where(rev == 1, ps, pe - le)))
            assert np.array_equal(lengths, np.where(part == 0, pe - ps, np.where(part == 1, ls, le))), "a sequence's length is not its part's"
            for p in range(3):
                assert ((part == p) & (rev == 0)).sum() >= 100 and ((part == p) & (rev == 1)).sum() >= 100, (cfg["name"], p)
            assert set(start % 32) == set(range(32)) and set(lengths % 4) == set(range(4)), cfg["name"]
            bit3 = [np.flatnonzero(np.frombuffer(reads[i], np.uint8) & 8) for i in take]
            covers = int(sum(((bit3[r] >= s) & (bit3[r] < s + n)).any() for r, s, n in zip(Q[:, 0], start, lengths)))
            if cfg["hpc"] and not cfg["valid_only"]:        # (the configuration that selects every position takes reads without such a character)
                assert covers >= 1, cfg["name"]
            long_reads = [j for j, i in enumerate(take) if len(reads[i]) > ALL_UPTO]
            for j in range(len(take)):
                want = np.arange(0, n_win[j], STRIDE if j in long_reads else 1)
                for p in range(3):
                    assert np.array_equal(Q[(Q[:, 0] == j) & (part == p), 1], want)
            np.savez_compressed(
                os.path.join(HERE, cfg["name"] + ".npz"), window_offsets=woff.astype(np.uint64), reversed=W[:, 1].astype(np.uint8),
                pos_start=W[:, 2].astype(np.uint32), pos_end=W[:, 3].astype(np.uint32), seq_length_start=W[:, 4].astype(np.uint32),
                seq_length_end=W[:, 5].astype(np.uint32), req_window=flat.astype(np.uint64), req_part=part.astype(np.uint32),
                lengths=lengths.astype(np.uint32), bitset=np.frombuffer(b"".join(blobs), dtype=np.uint8))
            manifest["configs"].append(dict(cfg, reads=take, left_out=int(left_out), n_windows=int(woff[-1]), n_requests=int(len(Q)),
                                            n_reversed_requests=int(rev.sum()), n_cover_bit3=covers, n_bases=int(lengths.sum())))
            print(cfg["name"], len(take), "reads", left_out, "left out", int(woff[-1]), "windows", len(Q), "requests", int(rev.sum()), "reversed", covers,
                  "cover a bit-3 character", int(lengths.sum()), "bases")
        manifest["soft_or_iupac_reads"] = int(soft_or_iupac)
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
