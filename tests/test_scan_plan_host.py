"""metamdbg_amd/csrc/scan_plan.hpp -- the host's plan of a scan: which path a batch takes, its regions and reserve, the limits of the
pre-filtered variant, grids, LDS padding, the placement of the reads the block kernel did not finish -- compiled for the host with the
address and undefined-behaviour sanitizers (tests/host/test_scan_plan.cpp): values pinned from the expressions as they stood inside
mdbg_scan and launch_scan, and the properties their comments state (the padding over every reserve and static size, the placement
against a restatement)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_plan_pinned_values_and_properties(tmp_path):
    exe = str(tmp_path / "test_scan_plan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "test_scan_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) checks", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) > 200_000                # the sweep of the LDS padding ran
