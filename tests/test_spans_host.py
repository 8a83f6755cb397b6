"""metamdbg_amd/csrc/spans_dev.hpp -- the run-start flags of a packed word, the j-th flag of a flag word, the coordinate map rle[j]
(tile, word, flag) and the composition of a window's ReadKminmer fields, as mdbg_kminmer_spans's kernels run them -- compiled for the
host with the address and undefined-behaviour sanitizers (tests/host/test_spans.cpp): every shape of flag word (empty, one flag, all 32,
flags only in the bottom or the top half, the partial last word); the map of seeded reads queried at every j in 0 .. L' against
EncoderRLE::execute's rule over the characters (runs across word, 64-word and tile borders, a run of 5000, reads that are one run, N
runs, "aA", IUPAC letters that share a code, an N next to a G); the composition against MDBG::getKminmers' arithmetic for forward,
reversed and tie windows, k = 2 included."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_select_map_and_composition(tmp_path):
    exe = str(tmp_path / "test_spans")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "test_spans.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) flag words in (\d+) shapes, (\d+) reads, (\d+) queries, (\d+) empty words, (\d+) empty tiles, (\d+) windows, (\d+) ties", r.stdout)
    assert m, r.stdout
    words, shapes, reads, queries, empty_words, empty_tiles, windows, ties = map(int, m.groups())
    assert shapes == 7 and words >= 200_000
    assert reads >= 700 and queries >= 500_000
    assert empty_words >= 100 and empty_tiles >= 1        # the inside of long runs: words and whole tiles without a run start
    assert windows >= 50_000 and ties >= 1_000
