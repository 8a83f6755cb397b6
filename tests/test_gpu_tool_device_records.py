"""`mdbg_tool readSelection` / `asmStep` with MDBG_TOOL_DEVICE_RECORDS=1: the records of read_data_init.txt and read_data_corrected.txt
are composed on the device (mdbg_minimizers_to_record_bytes) and the builder and writer threads only write them.  Every output file
must be the host builders', byte for byte; MDBG_TRACE says which path a run took."""
from __future__ import annotations

import os
import random
import struct
import subprocess

import numpy as np
import pytest

from metamdbg_amd import formats
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "metamdbg_amd", "bin", "mdbg_tool")
OUTPUTS = ("read_data_init.txt", "read_stats.txt", "read_data_corrected.txt", "repetitiveMinimizers.bin")
ON = "composed on the device"

HIFI = formats.Parameters(minimizer_size=15, kminmer_size=4, density=0.005, first_k=4, prev_k=4, hpc=True, data_type=0)
ONT = formats.Parameters(minimizer_size=15, kminmer_size=4, density=0.005, first_k=4, prev_k=4, hpc=False, data_type=1, correction_density=0.025)
ONT_ENV = {"MDBG_TOOL_REPETITIVE": os.path.join(H.GOLDEN, "ont_100", "repetitiveMinimizers.bin")}


def make_tmp(base, name, params: formats.Parameters, inputs: list[str]) -> str:
    tmp = os.path.join(str(base), name, "tmp")
    for d in ("", "filter", "smallContigs", "checkpoints"):
        os.makedirs(os.path.join(tmp, d), exist_ok=True)
    params.save(os.path.join(tmp, "parameters.gz"))
    with open(os.path.join(tmp, "input.txt"), "w") as f:
        f.write("\n".join(inputs) + "\n")
    return tmp


def run_tool(command, tmp, extra=(), env=None, min_q="0.000000", batch=1 << 20):
    e = dict(os.environ, MDBG_TRACE="1")
    for v in ("MDBG_TOOL_DEVICE_RECORDS", "MDBG_TOOL_DEVICE_PARSE"):
        e.pop(v, None)
    e.update(env or {})
    more = ["--min-abundance", "0"] if command == "asmStep" else []
    r = subprocess.run([TOOL, command, tmp, os.path.join(tmp, "read_data_init.txt"), os.path.join(tmp, "input.txt"), "--threads", "8",
                        "--min-read-quality", min_q, "--batch-bases", str(batch), *extra, *more], capture_output=True, text=True, env=e, timeout=120)
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


def both_ways(tmp_path, params, files, commands=("readSelection", "asmStep"), extra=(), env=None, on_env=None, **kw):
    """Every command with the switch off and on: the same files, byte for byte; the trace names the device path only when it is on."""
    result = {}
    for command in commands:
        outs = {}
        for name, e in (("host", {}), ("device", dict({"MDBG_TOOL_DEVICE_RECORDS": "1"}, **(on_env or {})))):
            tmp = make_tmp(tmp_path, f"{command}_{name}", params, files)
            err = run_tool(command, tmp, extra, dict(env or {}, **e), **kw)
            if name == "device":
                assert "device records: " in err and ON in err, err[-2000:]
                assert "falling back to the host builders" not in err
            else:
                assert "device records" not in err
            outs[name] = {f: open(os.path.join(tmp, f), "rb").read() for f in OUTPUTS if os.path.exists(os.path.join(tmp, f))}
        assert outs["host"].keys() == outs["device"].keys() and "read_data_init.txt" in outs["host"] and "read_stats.txt" in outs["host"]
        for f in outs["host"]:
            assert outs["host"][f] == outs["device"][f], (command, f)
        result[command] = outs["host"]
    if len(commands) == 2:                                                      # asmStep writes readSelection's files
        for f in result["readSelection"]:
            assert result["readSelection"][f] == result["asmStep"][f], f
    return result[commands[0]]


def write_fasta(tmp_path, n_files=3, n_reads=1500, seed0=100):
    files = []
    for f in range(n_files):
        path = str(tmp_path / f"in{f}.fasta")
        with open(path, "wb") as out:
            for i, s in enumerate(reads(seed0 + f, n_reads)):
                out.write(b">f%d_r%d\n" % (f, i) + s + b"\n")
        files.append(path)
    return files


def test_hifi_fasta(tmp_path):
    outs = both_ways(tmp_path, HIFI, write_fasta(tmp_path))
    assert len(outs["read_data_init.txt"]) > 23 * 4500                          # a record is 13 bytes and 10 per minimizer
    assert len(outs["read_data_corrected.txt"]) > 9 * 4500
    assert formats.parse_read_stats(outs["read_stats.txt"])["n_reads"] == 4500


def test_ont_fastq_with_a_quality_threshold_that_removes_reads(tmp_path):
    files = []
    for f in range(2):
        path = str(tmp_path / f"in{f}.fastq")
        q = np.random.default_rng(f)
        with open(path, "wb") as out:
            for i, s in enumerate(reads(200 + f, 1500)):
                level = 36 + int(q.integers(0, 38))                                 # phred 3 .. 40 and up to 5 more: some reads lie below 12, some above
                out.write(b"@f%d_r%d\n" % (f, i) + s + b"\n+\n" + q.integers(level, level + 6, len(s), dtype=np.uint8).tobytes() + b"\n")
        files.append(path)
    outs = both_ways(tmp_path, ONT, files, extra=["--skip-correction"], env=ONT_ENV, min_q="12.000000")
    rec = formats.parse_read_data_init(outs["read_data_init.txt"])
    assert len(rec) == 3000
    mean_q = np.array([struct.unpack("<f", struct.pack("<I", r["mean_quality_bits"]))[0] for r in rec])
    count = np.array([len(r["minimizers"]) for r in rec])
    assert (mean_q < 12).sum() > 100 and (mean_q >= 12).sum() > 100
    assert not count[mean_q < 12].any() and count[mean_q >= 12].sum() > 3000     # the threshold removed reads: their records keep length and quality


def test_together_with_the_device_parse(tmp_path):
    both_ways(tmp_path, HIFI, write_fasta(tmp_path, n_files=2, n_reads=800, seed0=500), on_env={"MDBG_TOOL_DEVICE_PARSE": "1"})


def test_more_than_a_group_of_batches(tmp_path):
    """--batch-bases small enough for more than 32 batches: the purge pass works on groups of 32 batches, each cut into its batches' pieces."""
    files = write_fasta(tmp_path, n_files=1, n_reads=1500, seed0=700)
    size = os.path.getsize(files[0])
    batch = 1 << 15
    assert size > 40 * batch
    both_ways(tmp_path, HIFI, files, batch=batch)
    err = run_tool("readSelection", make_tmp(tmp_path, "count", HIFI, files), env={"MDBG_TOOL_DEVICE_RECORDS": "1"}, batch=batch)
    n_batches = [int(line.split("]")[1].split()[0]) for line in err.splitlines() if " batches on " in line]
    assert n_batches and n_batches[0] > 32, err[-2000:]


def test_zero_reads(tmp_path):
    path = str(tmp_path / "empty.fasta")
    open(path, "wb").close()
    outs = both_ways(tmp_path, HIFI, [path])
    assert outs["read_data_init.txt"] == b"" and outs["read_data_corrected.txt"] == b""
