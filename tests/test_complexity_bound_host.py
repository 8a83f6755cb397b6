"""metamdbg_amd/csrc/complexity_dev.hpp -- the 2-mer bound of the low-complexity filter in its +-1 (Walsh-Hadamard) form -- compiled
for the host (tests/host/test_complexity_bound.cpp): every word's Q against a direct count of the 16 2-mers (more than a million
words: uniform, 30 % GC, homopolymers, every unit of period 2 - 6, every single-base change of poly-A), and the per-read decision
sum weight Q > 816 nW against the form it replaces, sum weight sq > 332 nW, on whole reads including reads steered onto the
threshold and 2 to either side of it (the sums are even: nothing lies nearer)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walsh_form_of_the_complexity_bound(tmp_path):
    exe = str(tmp_path / "test_complexity_bound")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "host", "test_complexity_bound.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) words, (\d+) reads \((\d+) suspect\), on the threshold -2/0/\+2: (\d+)/(\d+)/(\d+)", r.stdout)
    assert m, r.stdout
    words, reads, suspect, below, on, above = map(int, m.groups())
    assert words >= 1_000_000
    assert 0 < suspect < reads                      # both outcomes of the decision occur
    assert min(below, on, above) >= 10              # ... and reads on the threshold itself, and next to it on either side
