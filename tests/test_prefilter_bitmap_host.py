"""metamdbg_amd/csrc/prefilter.hpp -- the selected-key bitmap of the pre-filtered scan kernel: index function, key rule and builder --
compiled for the host (tests/host/test_prefilter_bitmap.cpp) and run over every 15-digit key: the counts of possible and selected keys
at density 0.005f, no selected key without its bit (at the kernel's geometry and at the tests' 2^10 bits), and the false-positive rate
of the kernel's geometry.  Once more as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_prefilter_bitmap.cpp")
FALSE_POSITIVE_64KB_ONE_PROBE = 0.0865          # enumerated on the CPU when the geometry was chosen


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_bitmap_over_every_key(tmp_path, flags):
    exe = str(tmp_path / "test_prefilter_bitmap")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-pthread"] + flags + [SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=1200)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^repeat-free 19131876$", r.stdout, re.M), r.stdout
    assert re.search(r"^canonical 9565938$", r.stdout, re.M), r.stdout
    assert re.search(r"^selected 47791$", r.stdout, re.M), r.stdout
    assert re.search(r"^helper mismatches 0$", r.stdout, re.M), r.stdout
    m = re.search(r"^log2_bits 19 set (\d+) missing 0 false-positive \d+ of 9518147 rate ([0-9.]+)$", r.stdout, re.M)
    assert m, r.stdout
    assert int(m.group(1)) * 4 <= 1 << 19                      # the fill gate of the kernel's launch passes at this density
    assert float(m.group(2)) < 1.5 * FALSE_POSITIVE_64KB_ONE_PROBE
    assert re.search(r"^log2_bits 10 set 1024 missing 0 ", r.stdout, re.M), r.stdout
