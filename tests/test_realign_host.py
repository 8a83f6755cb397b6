"""metamdbg_amd/csrc/realign_dev.hpp -- the oriented view of a thinned neighbour, a chain link's entries, the runs at both ends, the
normalisation step over tombstones, the entry kind -- compiled for the host as a stand-alone program (tests/host/test_realign.cpp), plain
and with the address and undefined-behaviour sanitizers, behind serial copies of the lane loops of realign.hip's chain, lists and compact
kernels and of the oriented fill of verify.hip's join, against a transcription of MinimizerChainer::computeChainingAlignment's list and
normalizeAlignment with std::vector::erase and against a plain reverse-complement copy: every pair of reads over {1, 2, 3} of at most 7
minimizers each and 10 together (8 under the sanitizers, which cost a factor of thirty) with every chain of two or more pairs in both
directions, a seeded sample of the longer pairs, chains of more links than a wave has lanes.  All pairs of 7 and 7 would be 10^7 pairs of
some hundred chains each: hours."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "test_realign.cpp")
LINE = (r"ok: (\d+) pairs, (\d+) chains, (\d+) reversed chains, (\d+)/(\d+) with/without a start run, (\d+)/(\d+) with/without an end run, (\d+) entries, (\d+) moves, "
        r"(\d+) erased, (\d+) cascades, (\d+) trips above one, (\d+) oriented reads, (\d+) oriented anchors, (\d+) mirrored runs")
# the smallest cascade with a chain the kernels would keep: tests/test_gpu_read_realign.py plants its shape (a run of one minimizer, one
# copy more in the neighbour, the chain stepping over it)
CASCADE = ("cascade: target 1 1 1 1 | neighbour 1 1 1 1 1\n"
           "cascade chain: (0,0) (1,1) (2,3) (3,4)\n"
           "cascade raw: (0,0) (1,1) (-1,2) (2,3) (3,4)\n"
           "cascade final: (0,0) (1,1) (2,2) (3,3) (-1,4)\n")


@pytest.mark.parametrize("flags,together,pairs", [((), 10, 478535), (("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"), 8, 65192)], ids=["plain", "sanitized"])
def test_rules_behind_the_lane_loops(tmp_path, flags, together, pairs):
    exe = str(tmp_path / "test_realign")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, SOURCE, "-o", exe], check=True)
    r = subprocess.run([exe, str(together)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert r.stdout.startswith("cascade: target ") and (together < 9 or r.stdout.startswith(CASCADE)), r.stdout      # (its 9 minimizers: not among the pairs of 8)
    m = re.search(LINE, r.stdout)
    assert m, r.stdout
    (n_pairs, chains, reversed_chains, start, no_start, end, no_end, entries, moves, erased, cascades, trips, oriented_reads, oriented_anchors,
     mirrored) = map(int, m.groups())
    assert n_pairs == pairs          # the pairs of at most `together` minimizers, the 1200 sampled ones, the 20 long ones
    assert chains > 0 and 0 < reversed_chains < chains and start > 0 and no_start > 0 and end > 0 and no_end > 0 and start + no_start == chains
    assert entries > 0 and moves > 0 and erased > 0 and cascades > 0 and trips > 0
    assert oriented_reads == 800 and oriented_anchors > 0 and mirrored > 0
