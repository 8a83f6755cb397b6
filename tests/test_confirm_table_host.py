"""metamdbg_amd/csrc/prefilter.hpp -- the selected-key table the pre-filtered scan kernel takes its candidates' verdicts from: index
function, bucket layout, builder and look-up -- compiled for the host (tests/host/test_confirm_table.cpp) and run over every 15-digit
key: at density 0.005f with the kernel's 2^16 buckets every possible key's answer is prefilter_key_selected and no bucket overflows; at
0.01f the buckets of more than seven keys answer "ask the hash" and every other answer is exact; in the tests' geometries (2^13 and 2^10
buckets) marked buckets and exact ones mix.  Once more as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_confirm_table.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_table_over_every_key(tmp_path, flags):
    exe = str(tmp_path / "test_confirm_table")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-pthread"] + flags + [SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=1200)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    cases = re.split(r"^case ", r.stdout, flags=re.M)[1:]
    assert [c.split("\n")[0].split(" threshold")[0] for c in cases] == [
        "density 0.005 log2_buckets 16", "density 0.01 log2_buckets 16", "density 0.005 log2_buckets 13", "density 0.005 log2_buckets 10"]
    for c in cases:
        assert re.search(r"^  possible 9565938 selected (47791|95524)$", c, re.M), c
        # every answer exact or ASK, ASK from marked buckets only, builder and probe agree, empty slots match nothing
        assert re.search(r" wrong 0 ask-mismatch 0 index-mismatch 0 empty-hit 0 filler-bad 0$", c, re.M), c
        assert re.search(r"^  ok$", c, re.M), c
    # the kernel's geometry at the bench's density: no bucket holds more than seven keys, every selected key answers YES
    assert re.search(r" max 7$", cases[0], re.M) and "overflowed 0 (by count 0)" in cases[0], cases[0]
    assert "answers yes 47791 ask 0 " in cases[0], cases[0]
    # at 0.01f a handful of buckets overflow; their keys, and no others, ask
    m = re.search(r"overflowed (\d+) \(by count (\d+)\)", cases[1])
    assert m and 0 < int(m.group(1)) == int(m.group(2)) <= 32, cases[1]
    assert int(re.search(r"answers yes (\d+) ask (\d+) ", cases[1]).group(2)) > 0
    # the tests' geometries: 2^13 buckets mix exact answers and ASK, 2^10 buckets all overflow
    m = re.search(r"answers yes (\d+) ask (\d+) ", cases[2])
    assert int(m.group(1)) > 1000 and int(m.group(2)) > 1000, cases[2]
    assert "overflowed 1024 (by count 1024)" in cases[3] and "answers yes 0 ask 9565938 " in cases[3], cases[3]
