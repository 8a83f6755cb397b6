"""metamdbg_amd/host/ordered_place.hpp and bgzf_slabs.hpp -- where readSelection's out-of-order batches go in their file, and how a BGZF
file is cut into slabs of text for the device parse -- compiled for the host (tests/host/test_tool_placement.cpp) and driven without a
library or a GPU: batches delivered in reverse, interleaved from three consumers, of zero bytes, alone, and 10 000 of random size; BGZF
files of one block, with empty blocks, with a block larger than a batch, with records that end on a block's edge, span three blocks or
are longer than a batch, and a batch of one byte.  Once more as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_tool_placement.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_placement_and_bgzf_slabs(tmp_path, flags):
    exe = str(tmp_path / "test_tool_placement")
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + [SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "FAILED" not in r.stdout and r.stdout.rstrip().endswith("all ok")
    cases = re.findall(r"^case (\w+) ([\w-]+) ok", r.stdout, re.M)
    assert [n for k, n in cases if k == "placement"] == ["reverse", "three-consumers", "zero-byte-items", "all-zero-bytes", "single-item", "10000-random"]
    bgzf = [n for k, n in cases if k == "bgzf"]
    assert [n for n in bgzf if not n.startswith("random-")] == [
        "one-block", "one-block-large-batch", "empty-blocks", "only-empty-blocks", "block-larger-than-batch",
        "record-spans-three-blocks-and-one-ends-on-an-edge", "records-end-on-every-edge", "record-longer-than-batch",
        "first-record-longer-than-batch", "batch-of-one", "batch-of-one-record-of-two-blocks", "batch-of-one-record-of-three-blocks"]
    assert len([n for n in bgzf if n.startswith("random-")]) == 200
