"""metamdbg_amd/csrc/select_dev.hpp -- the rank key, the counter step, the score of a match list, where a record of the alignment file
starts -- compiled for the host behind a serial copy of select_kernel's lane loop (tests/host/test_select.cpp), plain and again with the
address and undefined-behaviour sanitizers, against a transcription of the reference's heap procedure (std::priority_queue with
AlignmentScoreComparator, candidates fed in ascending read index): every assignment of a score from {-1, 0, 1, 2} and a non-empty subset of
4 positions to up to 3 candidates and a seeded sample of the assignments to 4, 5 and 6 (the full enumeration is 60^6: bounded, see the
program) at coverage 1, 2 and 3; seeded sets of 1 - 300 candidates at coverage 1, 20 and 255; list lengths 1, 63, 64, 65, 128 and 129;
a counter that saturates at 255; the rank key over INT32_MIN, -1, 0, 1, INT32_MAX; the record start past 2^32."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_lane_loop_against_the_heaps(tmp_path, flags):
    exe = str(tmp_path / "test_select")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + [os.path.join(ROOT, "tests", "host", "test_select.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) cases, (\d+) candidates, (\d+) selected, (\d+) pushed and evicted everywhere, (\d+) ties at the cut, (\d+) saturated steps, "
                 r"(\d+) partial trips, (\d+) lists above one trip", r.stdout)
    assert m, r.stdout
    cases, candidates, selected, evicted, ties, saturated, partial, long_lists = map(int, m.groups())
    print(r.stdout)
    assert cases >= 3 * (60 + 60 ** 2 + 60 ** 3 + 3 * 50000) + 3 * 60 + 3 + 1
    assert 0 < selected < candidates
    assert evicted > 0 and ties > 0 and saturated > 0 and partial > 0 and long_lists > 0
