"""metamdbg_amd/csrc/segments_dev.hpp -- how a long read is cut into the views the block-structured scan takes one wave each -- compiled
for the host with the address and undefined-behaviour sanitizers (tests/host/test_scan_segments.cpp): the run starts of every 2048-base
tile, the compressed offset c_s of every segment, the windows each view owns (they partition [0, C)) and the verdict "unsegmentable",
against a character-by-character homopolymer compression of random reads, run-free reads, homopolymers at, before and across every
cut (every length 1 .. 40 and chosen lengths up to 5000: around 2033 - 2035, one tile, two tiles), and lengths 2048 m + {-1, 0, 1}."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segment_arithmetic_against_direct_compression(tmp_path):
    exe = str(tmp_path / "test_scan_segments")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "test_scan_segments.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) reads, (\d+) views, (\d+) unsegmentable, (\d+) cuts inside a run", r.stdout)
    assert m, r.stdout
    reads, views, unsegmentable, in_run = map(int, m.groups())
    assert reads >= 10_000 and views > 2 * reads
    assert 0 < unsegmentable < reads                # both verdicts occur
    assert in_run >= 100                            # ... and cuts that fall inside a run
