"""`mdbg_tool readSelection` with MDBG_TOOL_DEVICE_PARSE=1 on BGZF input: the compressed bytes travel to the device slab by slab, are
inflated there (mdbg_bytes_inflate_bgzf), cut behind their last whole record (mdbg_fastx_whole_records) and taken apart
(mdbg_reads_from_fastx_bytes).  Every output file must be the host feed's, byte for byte, and MDBG_TRACE must say "inflated on the
device"; gzip that is not pure BGZF falls back to the host feed with the reason; a block that does not inflate in mid-run stops the
tool with the library's message."""
from __future__ import annotations

import gzip
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
INFLATED = "inflated on the device"

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


def fasta_crlf(seed, n, tag):
    return b"".join(b">%s_r%d\r\n" % (tag, i) + b"".join(s[at:at + 70] + b"\r\n" for at in range(0, len(s), 70)) for i, s in enumerate(reads(seed, n)))


def fastq(seed, n, tag):
    q = np.random.default_rng(seed + 1000)
    return b"".join(b"@%s_r%d\n" % (tag, i) + s + b"\n+\n" + q.integers(36, 80, len(s), dtype=np.uint8).tobytes() + b"\n" for i, s in enumerate(reads(seed, n)))


def write(path, raw):
    with open(str(path), "wb") as f:
        f.write(raw)
    return str(path)


def both_ways(tmp_path, params, files, n_reads, extra=(), env=None, expect=INFLATED):
    outs = {}
    for name, e in (("host", {}), ("device", {"MDBG_TOOL_DEVICE_PARSE": "1"})):
        tmp = make_tmp(tmp_path, name, params, files)
        r = run_tool(tmp, extra, dict(env or {}, **e))
        assert r.returncode == 0, r.stderr[-2000:]
        if name == "device":
            assert expect in r.stderr, r.stderr[-2000:]
            if expect != INFLATED:
                assert INFLATED not in r.stderr
            outs["trace"] = r.stderr
        else:
            assert "device parse" not in r.stderr
        outs[name] = {f: open(os.path.join(tmp, f), "rb").read() for f in OUTPUTS if os.path.exists(os.path.join(tmp, f))}
    assert outs["host"].keys() == outs["device"].keys() and "read_data_init.txt" in outs["host"]
    for f in outs["host"]:
        assert outs["host"][f] == outs["device"][f], f
    # not an empty comparison: a record is 13 bytes and 10 per minimizer, and reads of 300 - 3000 bases hold more than one on average
    assert len(outs["host"]["read_data_init.txt"]) > 23 * n_reads
    return outs


def slabs_of(trace):
    m = re.search(r"(\d+) BGZF block\(s\) of (\d+) file\(s\) inflated on the device in (\d+) slab\(s\)", trace)
    assert m, trace[-2000:]
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def test_three_crlf_fasta_files(tmp_path):
    files, n_blocks = [], 0
    for f in range(3):
        raw = formats.bgzf_compress(fasta_crlf(100 + f, 1500, b"f%d" % f), block=0xFF00)
        n_blocks += len(formats.bgzf_blocks(raw))
        files.append(write(tmp_path / f"in{f}.fasta.gz", raw))
    outs = both_ways(tmp_path, HIFI, files, 3 * 1500)
    assert "read_data_corrected.txt" in outs["host"]
    blocks, n_files, slabs = slabs_of(outs["trace"])
    assert (blocks, n_files) == (n_blocks, 3) and slabs >= 3 * 2        # 2.5 MB of text a file, slabs of 1 MB


def test_two_fastq_files_in_small_blocks(tmp_path):
    files, n_text = [], 0
    for f in range(2):
        text = fastq(200 + f, 1500, b"f%d" % f)
        n_text += len(text)
        files.append(write(tmp_path / f"in{f}.fastq.gz", formats.bgzf_compress(text, block=3000)))
    outs = both_ways(tmp_path, ONT, files, 2 * 1500, **ONT_ARGS)
    blocks, n_files, slabs = slabs_of(outs["trace"])
    assert n_files == 2 and blocks >= n_text // 3000 and slabs >= n_text >> 20     # records cross every block and slab border


def test_plain_and_bgzf_in_one_list(tmp_path):
    files = [write(tmp_path / "plain.fasta", fasta_crlf(300, 700, b"p")),
             write(tmp_path / "blocked.fasta.gz", formats.bgzf_compress(fasta_crlf(301, 700, b"b"), block=0xFF00)),
             write(tmp_path / "plain2.fasta", fasta_crlf(302, 300, b"q"))]
    outs = both_ways(tmp_path, HIFI, files, 1700)
    assert "taken apart on the device" in outs["trace"] and slabs_of(outs["trace"])[1] == 1


def test_gzip_that_is_not_bgzf_falls_back(tmp_path):
    text = fastq(400, 400, b"g")
    plain_gzip = write(tmp_path / "plain.fastq.gz", gzip.compress(text, 6))
    outs = both_ways(tmp_path, ONT, [plain_gzip], 400, expect="falling back to the host feed", **ONT_ARGS)
    assert "plain.fastq.gz is gzip but not BGZF" in outs["trace"]
    tail = write(tmp_path / "tail.fastq.gz", formats.bgzf_compress(text[:len(text) // 2], block=0xFF00, eof_marker=False) + gzip.compress(text[len(text) // 2:], 6))
    assert formats.bgzf_blocks(open(tail, "rb").read()) is None
    outs = both_ways(tmp_path / "tail", ONT, [tail], 400, expect="falling back to the host feed", **ONT_ARGS)
    assert "tail.fastq.gz is gzip but not BGZF" in outs["trace"]


def test_a_damaged_block_in_mid_run_stops_the_tool(tmp_path):
    text = fasta_crlf(500, 1500, b"d")
    raw = bytearray(formats.bgzf_compress(text, block=0xFF00))
    blocks = formats.bgzf_blocks(bytes(raw))
    i = len(blocks) // 2                                               # far behind the prefix the plan looks at on the host
    assert sum(b[2] for b in blocks[:i]) > 1 << 20
    src, csize, isize, crc = blocks[i]
    raw[src + csize // 2] ^= 0x20
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(raw[src:src + csize]))
        bad = not d.eof or len(out) != isize or zlib.crc32(out) & 0xFFFFFFFF != crc
    except zlib.error:
        bad = True
    assert bad, "the changed byte must make the block wrong by zlib's account"
    assert formats.bgzf_blocks(bytes(raw)) is not None                 # still pure BGZF by its headers
    path = write(tmp_path / "damaged.fasta.gz", bytes(raw))
    r = run_tool(make_tmp(tmp_path, "device", HIFI, [path]), env={"MDBG_TOOL_DEVICE_PARSE": "1"})
    assert r.returncode != 0
    assert "mdbg_bytes_inflate_bgzf: block" in r.stderr and "does not decode" in r.stderr, r.stderr[-2000:]
    assert "falling back" not in r.stderr
