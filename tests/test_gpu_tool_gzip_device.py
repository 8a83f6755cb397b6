"""`mdbg_tool readSelection` with MDBG_TOOL_DEVICE_PARSE=1 on ordinary gzip input (gzip -6, concatenated members): worker threads find one
deflate block header per MDBG_TOOL_GZIP_CHUNK_KB of compressed file, the consumers inflate groups of chunks on the device
(mdbg_bytes_inflate_gzip), cut behind the last whole record (mdbg_fastx_whole_records) and carry the rest to the next slab
(mdbg_bytes_copy).  Every output file must be the host feed's, byte for byte, and MDBG_TRACE must name the device gzip path; a stored-only
.gz holds no header the search finds and takes the host feed, with the reason."""
from __future__ import annotations

import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from metamdbg_amd import formats
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "metamdbg_amd", "bin", "mdbg_tool")
OUTPUTS = ("read_data_init.txt", "read_stats.txt", "read_data_corrected.txt", "repetitiveMinimizers.bin")
DEVICE_GZIP = "gzip file(s) inflated on the device"

HIFI = formats.Parameters(minimizer_size=15, kminmer_size=4, density=0.005, first_k=4, prev_k=4, hpc=True, data_type=0)
ONT = formats.Parameters(minimizer_size=15, kminmer_size=4, density=0.005, first_k=4, prev_k=4, hpc=False, data_type=1, correction_density=0.025)
ONT_ARGS = dict(extra=["--skip-correction"], env={"MDBG_TOOL_REPETITIVE": os.path.join(H.GOLDEN, "ont_100", "repetitiveMinimizers.bin")})


def make_tmp(base, name, params: formats.Parameters, inputs: list[str]) -> str:
    tmp = os.path.join(str(base), name, "tmp")
    for d in ("", "filter", "smallContigs", "checkpoints"):
        os.makedirs(os.path.join(tmp, d), exist_ok=True)
    params.save(os.path.join(tmp, "parameters.gz"))
    with open(os.path.join(tmp, "input.txt"), "w") as f:
        f.write("\n".join(inputs) + "\n")
    return tmp


def run_tool(tmp, extra=(), env=None):
    e = dict(os.environ, MDBG_TRACE="1")
    e.pop("MDBG_TOOL_DEVICE_PARSE", None)
    e.update(env or {})
    return subprocess.run([TOOL, "readSelection", tmp, os.path.join(tmp, "read_data_init.txt"), os.path.join(tmp, "input.txt"), "--threads", "8",
                           "--min-read-quality", "0.000000", "--batch-bases", str(1 << 20), *extra], capture_output=True, text=True, env=e, timeout=120)


def reads(seed, n):
    rng = np.random.default_rng(seed)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), 1 << 17)
    out = []
    for i in range(n):
        L = int(rng.integers(300, 3000))
        at = int(rng.integers(0, len(genome) - L))
        s = genome[at:at + L].tobytes()
        if i % 11 == 3:
            cut = int(rng.integers(0, L - 40))
            s = s[:cut] + s[cut:cut + 20].lower() + b"N" + s[cut + 21:]
        out.append(s)
    return out


def fasta(seed, n, tag):
    return b"".join(b">%s_r%d\n" % (tag, i) + b"".join(s[at:at + 70] + b"\n" for at in range(0, len(s), 70)) for i, s in enumerate(reads(seed, n)))


def fastq(seed, n, tag):
    q = np.random.default_rng(seed + 1000)
    return b"".join(b"@%s_r%d\n" % (tag, i) + s + b"\n+\n" + q.integers(36, 80, len(s), dtype=np.uint8).tobytes() + b"\n" for i, s in enumerate(reads(seed, n)))


def gzip_member(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def write(path, raw):
    with open(str(path), "wb") as f:
        f.write(raw)
    return str(path)


def both_ways(tmp_path, params, files, n_reads, extra=(), env=None):
    outs = {}
    for name, e in (("host", {}), ("device", {"MDBG_TOOL_DEVICE_PARSE": "1", "MDBG_TOOL_GZIP_CHUNK_KB": "16"})):
        tmp = make_tmp(tmp_path, name, params, files)
        r = run_tool(tmp, extra, dict(env or {}, **e))
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name + " trace"] = r.stderr
        outs[name] = {f: open(os.path.join(tmp, f), "rb").read() for f in OUTPUTS if os.path.exists(os.path.join(tmp, f))}
    assert "device parse" not in outs["host trace"]
    assert outs["host"].keys() == outs["device"].keys() and "read_data_init.txt" in outs["host"]
    for f in outs["host"]:
        assert outs["host"][f] == outs["device"][f], f
    assert len(outs["host"]["read_data_init.txt"]) > 23 * n_reads       # not an empty comparison
    return outs


def device_path(trace):
    m = re.search(r"(\d+) chunk\(s\) of (\d+) gzip file\(s\) inflated on the device in (\d+) call\(s\), (\d+) slab\(s\)", trace)
    assert m, trace[-3000:]
    return tuple(int(g) for g in m.groups())


def test_a_fasta_compressed_with_gzip_6(tmp_path):
    text = fasta(600, 1900, b"a")                              # about 3 MB of text
    raw = gzip_member(text, 6)
    outs = both_ways(tmp_path, HIFI, [write(tmp_path / "reads.fasta.gz", raw)], 1900)
    assert "read_data_corrected.txt" in outs["host"]
    assert DEVICE_GZIP in outs["device trace"] and "falling back" not in outs["device trace"]
    chunks, files, calls, slabs = device_path(outs["device trace"])
    assert files == 1 and calls >= 3 and slabs >= 3            # slabs of 1 MB of text: records cross slab and call borders
    assert chunks >= len(raw) // (2 * 16384)                   # a start in most 16 KB pieces of the file


def test_a_fastq_of_two_concatenated_members(tmp_path):
    text = fastq(700, 900, b"q")
    half = text.index(b"\n@q_r450\n") + 1
    raw = gzip_member(text[:half], 6) + gzip_member(text[half:], 1)
    outs = both_ways(tmp_path, ONT, [write(tmp_path / "reads.fastq.gz", raw)], 900, **ONT_ARGS)
    assert DEVICE_GZIP in outs["device trace"] and "falling back" not in outs["device trace"]
    assert device_path(outs["device trace"])[1] == 1


def test_a_stored_only_gz_takes_the_host_feed(tmp_path):
    text = fasta(800, 300, b"s")
    raw = gzip_member(text, 0)
    outs = both_ways(tmp_path, HIFI, [write(tmp_path / "stored.fasta.gz", raw)], 300)
    trace = outs["device trace"]
    assert "falling back to the host feed" in trace and "stored.fasta.gz is gzip but not BGZF" in trace and "no deflate block header" in trace
    assert DEVICE_GZIP not in trace
