"""metamdbg_amd/csrc/murmur.hpp -- the candidate hash with the finalisers' upper half shared (kmer_hash32_hi_shared, _x2) -- compiled
for the host (tests/host/test_murmur_shared_hi.cpp) and run over every key v < 2^32: bit-identical to kmer_hash32_hi_merged wherever
the guard word passes; 65 keys fail it, 14 of them below 2^30 (reachable at l = 15), none of those free of equal adjacent digits --
which is why the scan kernel drops the guard under homopolymer compression at l = 15 -- and exactly one repeat-free key fails among
the 16-digit ones (l = 16, where the guard stays)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BELOW_2_30 = [18684438, 62257441, 95494466, 172304494, 421419016, 498229044, 531466069, 550150507, 583387532, 626960535, 660197560,
              737007588, 986122110, 1062932138]


def _list(out, head):
    m = re.search(r"^" + re.escape(head) + r" (\d+):((?: \d+)*)$", out, re.M)
    assert m, (head, out)
    vals = [int(x) for x in m.group(2).split()]
    assert len(vals) == int(m.group(1))
    return vals


def test_shared_upper_half_over_every_key(tmp_path):
    exe = str(tmp_path / "test_murmur_shared_hi")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-pthread",
                    os.path.join(ROOT, "tests", "host", "test_murmur_shared_hi.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=1200)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^mismatches 0$", r.stdout, re.M), r.stdout
    m = re.search(r"^x2 checked (\d+) mismatches 0$", r.stdout, re.M)
    assert m and int(m.group(1)) >= (1 << 26), r.stdout
    failing = _list(r.stdout, "failing")
    assert len(failing) == 65
    assert [v for v in failing if v < (1 << 30)] == BELOW_2_30
    assert _list(r.stdout, "l 15 below") == BELOW_2_30
    assert _list(r.stdout, "l 15 repeat-free") == []
    assert _list(r.stdout, "l 16 below") == failing
    assert len(_list(r.stdout, "l 16 repeat-free")) == 1
    # l = 13 and 14: subsets of the l = 15 list, so repeat-free ones there would be (prefix-wise) no contradiction -- listed, and
    # consistent with the list above
    for l in (13, 14):
        below = _list(r.stdout, "l %d below" % l)
        assert below == [v for v in BELOW_2_30 if v < (1 << (2 * l))]
        assert set(_list(r.stdout, "l %d repeat-free" % l)) <= set(below)
