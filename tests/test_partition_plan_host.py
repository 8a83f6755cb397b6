"""metamdbg_amd/csrc/partition_plan.hpp -- the plan of the first pass's radix split: the share of a segment a block takes, blocks per
segment and grids per level -- compiled for the host with the address and undefined-behaviour sanitizers
(tests/host/test_partition_plan.cpp): values pinned from the expressions as they stood inside PartRun::split_group, and the properties of
the shares (every record of every segment in exactly one share, every share but a segment's last a multiple of the tile).  Likewise bucket
bits, levels, the slot choice, key-group bits and the per-level table of the first pass and of the owner of a sharded pass: pinned at the
seams from PartRun::bits_for / levels_for / plan / init and part_owner_reduce as they stood, and the properties of a level table."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_partition_plan_pinned_values_and_properties(tmp_path):
    exe = str(tmp_path / "test_partition_plan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "test_partition_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) checks", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) > 100_000                # the sweep over records, segments, tiles, shares and levels ran
