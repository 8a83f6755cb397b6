"""The gzip chunk decoder of metamdbg_amd/csrc/deflate_core.hpp (gz_step) -- what lane 0 of gzip_decode_kernel runs -- compiled for the
host behind a serial copy of the wave loop, the window chain, the translation and the CRC by pieces (tests/host/test_gzip_core.cpp),
under the address and undefined-behaviour sanitizers: every corpus item at every true block start (zlib's inflate(Z_BLOCK)) and at every
third one byte for byte against zlib, then seeded mutants that must give zlib's bytes or be refused, and the header search
mdbg_host::gzip_find_block against the true headers."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gzip_core_against_zlib(tmp_path):
    out = str(tmp_path / "test_gzip_core")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "host", "test_gzip_core.cpp"), "-o", out, "-lz"], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.match(r"ok (\d+) items, (\d+) decodes of (\d+) chunks, (\d+) mutants \((\d+) still inflate, (\d+) refused\), (\d+) header searches", r.stdout)
    assert m, r.stdout
    items, decodes, chunks, mutants, still, refused, found = map(int, m.groups())
    assert items >= 14 and decodes == 3 * items and chunks > 100
    assert still > 0 and refused > 0 and still + refused == mutants      # both sides are exercised
    assert found >= 6
