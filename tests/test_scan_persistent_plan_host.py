"""metamdbg_amd/csrc/scan_plan.hpp -- the plan of the pre-filtered scan's persistent launch: the grid, the clipping of the last run, runs
drawn from one counter by any interleaving of waves covering every read exactly once, the even deal of runs to regions -- compiled for
the host plain and with the address and undefined-behaviour sanitizers (tests/host/test_scan_persistent_plan.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_scan_persistent_plan(tmp_path, flags):
    exe = str(tmp_path / "test_scan_persistent_plan")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, os.path.join(ROOT, "tests", "host", "test_scan_persistent_plan.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) checks", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) > 1_000_000                # the interleavings ran
