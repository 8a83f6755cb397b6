"""`mdbg_tool readSelection` with MDBG_TOOL_DEVICE_PARSE=1: plain FASTA / FASTQ files travel to the device as text, slab by slab, and
are taken apart there (mdbg_reads_from_fastx_bytes).  Every output file must be the host feed's, byte for byte; MDBG_TRACE says which
path a run took; an input the device parse refuses (multi-line FASTQ) falls back to the host feed."""
from __future__ import annotations

import os
import random
import subprocess

import numpy as np
import pytest

from metamdbg_amd import formats
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "metamdbg_amd", "bin", "mdbg_tool")
OUTPUTS = ("read_data_init.txt", "read_stats.txt", "read_data_corrected.txt", "repetitiveMinimizers.bin")


def make_tmp(base, name, params: formats.Parameters, inputs: list[str]) -> str:
    tmp = os.path.join(str(base), name, "tmp")
    for d in ("", "filter", "smallContigs", "checkpoints"):
        os.makedirs(os.path.join(tmp, d), exist_ok=True)
    params.save(os.path.join(tmp, "parameters.gz"))
    with open(os.path.join(tmp, "input.txt"), "w") as f:
        f.write("\n".join(inputs) + "\n")
    return tmp


def read_selection(tmp, extra=(), env=None):
    e = dict(os.environ, MDBG_TRACE="1")
    e.pop("MDBG_TOOL_DEVICE_PARSE", None)
    e.update(env or {})
    r = subprocess.run([TOOL, "readSelection", tmp, os.path.join(tmp, "read_data_init.txt"), os.path.join(tmp, "input.txt"), "--threads", "8",
                        "--min-read-quality", "0.000000", "--batch-bases", str(1 << 20), *extra], capture_output=True, text=True, env=e, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def reads(seed, n):
    rng = random.Random(seed)
    genome = np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", np.uint8), 1 << 17)
    out = []
    for i in range(n):
        L = rng.randrange(300, 3000)
        at = rng.randrange(0, len(genome) - L)
        s = genome[at:at + L].tobytes()
        if i % 11 == 3:
            cut = rng.randrange(0, L - 40)
            s = s[:cut] + s[cut:cut + 20].lower() + b"N" + s[cut + 21:]
        out.append(s)
    return out


def both_ways(tmp_path, params, files, n_reads, extra=(), env=None, expect="taken apart on the device"):
    outs = {}
    for name, e in (("host", {}), ("device", {"MDBG_TOOL_DEVICE_PARSE": "1"})):
        tmp = make_tmp(tmp_path, name, params, files)
        err = read_selection(tmp, extra, dict(env or {}, **e))
        if name == "device":
            assert expect in err, err[-2000:]
        else:
            assert "device parse" not in err
        outs[name] = {f: open(os.path.join(tmp, f), "rb").read() for f in OUTPUTS if os.path.exists(os.path.join(tmp, f))}
    assert outs["host"].keys() == outs["device"].keys() and "read_data_init.txt" in outs["host"]
    for f in outs["host"]:
        assert outs["host"][f] == outs["device"][f], f
    # not an empty comparison: a record is 13 bytes and 10 per minimizer, and reads of 300 - 3000 bases hold more than one on average
    assert len(outs["host"]["read_data_init.txt"]) > 23 * n_reads
    return outs


HIFI = formats.Parameters(minimizer_size=15, kminmer_size=4, density=0.005, first_k=4, prev_k=4, hpc=True, data_type=0)
ONT = formats.Parameters(minimizer_size=15, kminmer_size=4, density=0.005, first_k=4, prev_k=4, hpc=False, data_type=1, correction_density=0.025)


def test_multi_line_crlf_fasta(tmp_path):
    files = []
    for f in range(3):
        path = str(tmp_path / f"in{f}.fasta")
        with open(path, "wb") as out:
            for i, s in enumerate(reads(100 + f, 1500)):
                out.write(b">f%d_r%d\r\n" % (f, i) + b"".join(s[at:at + 70] + b"\r\n" for at in range(0, len(s), 70)))
        files.append(path)
    outs = both_ways(tmp_path, HIFI, files, 3 * 1500)
    assert "read_data_corrected.txt" in outs["host"]


def test_four_line_fastq_with_qualities(tmp_path):
    files = []
    for f in range(2):
        path = str(tmp_path / f"in{f}.fastq")
        q = np.random.default_rng(f)
        with open(path, "wb") as out:
            for i, s in enumerate(reads(200 + f, 1500)):
                out.write(b"@f%d_r%d\n" % (f, i) + s + b"\n+\n" + q.integers(36, 80, len(s), dtype=np.uint8).tobytes() + b"\n")
        files.append(path)
    both_ways(tmp_path, ONT, files, 2 * 1500, extra=["--skip-correction"],
              env={"MDBG_TOOL_REPETITIVE": os.path.join(H.GOLDEN, "ont_100", "repetitiveMinimizers.bin")})


def test_multi_line_fastq_falls_back(tmp_path):
    path = str(tmp_path / "wrapped.fastq")
    q = np.random.default_rng(5)
    with open(path, "wb") as out:
        for i, s in enumerate(reads(300, 400)):
            qual = q.integers(36, 80, len(s), dtype=np.uint8).tobytes()
            out.write(b"@r%d\n" % i + b"".join(s[at:at + 80] + b"\n" for at in range(0, len(s), 80)) + b"+\n" +
                      b"".join(qual[at:at + 80] + b"\n" for at in range(0, len(s), 80)))
    both_ways(tmp_path, HIFI, [path], 400, expect="falling back to the host feed")
