"""metamdbg_amd/csrc/deflate_core.hpp -- the serial core of the device's DEFLATE decoder -- compiled for the host and checked against
zlib under the address and undefined-behaviour sanitizers (tests/host/test_deflate_core.cpp): every corpus item byte for byte, then
seeded mutants (bit flips, truncation, a wrong isize) on which the core must agree with zlib's raw inflate or report an error."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_deflate_core_against_zlib(tmp_path):
    out = str(tmp_path / "test_deflate_core")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "host", "test_deflate_core.cpp"), "-o", out, "-lz"], check=True)
    r = subprocess.run([out, "20240611", "2400"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    m = re.match(r"ok (\d+) members, (\d+) mutants \((\d+) still inflate, (\d+) refused\)", r.stdout)
    assert m, r.stdout
    members, mutants, still, refused = map(int, m.groups())
    assert members >= 45 and mutants >= 2000
    assert still > 100 and refused > 100            # both sides of the rule are exercised
