"""metamdbg_amd/host/graph_plan.hpp -- where `mdbg_tool graph` cuts a read set into pieces (and its two refusals), which reads a rank takes, which
bytes of read_data_corrected.txt a range of records is, which record files a pass writes -- compiled for the host with the address and
undefined-behaviour sanitizers (tests/host/test_graph_plan.cpp): every value against the expressions as they stood inside mdbg_tool.cpp,
over chosen offsets and a few thousand random read sets, and the properties of a set of cuts."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_graph_plan_equals_the_expressions_it_replaced(tmp_path):
    exe = str(tmp_path / "test_graph_plan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "test_graph_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) checks", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) > 100_000                # the chosen offsets and the random read sets ran
