"""metamdbg_amd/csrc/verify_dev.hpp -- the run of neighbour indexes a target minimizer meets, the gaps and the summary of a chain, kept or not,
the identity and its table -- and the chain rules of mapper_dev.hpp it reuses, compiled for the host with the address and
undefined-behaviour sanitizers behind serial copies of the count, fill and chain lane loops and of lane 0's walk in verify.hip
(tests/host/test_verify.cpp), against a brute-force transcription of filterAlignments' join and MinimizerChainer.hpp with the reference's own
types (float scores): every multiset of up to 5 anchors over a grid of 3 x 3 positions and both strands at bands 1, 2 and 5, seeded pairs of
reads of 1 - 400 anchors at bands 1, 5, 62, 64, 65 and 130, the table of smallest passing n_matches by binary search against the full scan,
and the fixture's _identity floats bit for bit."""
import os
import re
import subprocess

import numpy as np

from tests import verify_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rules_behind_the_lane_loops(tmp_path):
    exe = str(tmp_path / "test_verify")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "test_verify.cpp"), "-o", exe], check=True)
    lines = []
    for cfg in vm.fixture_manifest()["configs"]:
        d = vm.load_fixture(cfg["name"])
        rows = vm.fixture_verification(d)["rows"]
        for s in np.flatnonzero(d["row_chain"]):
            lines.append(f"{cfg['minimizer_size']} {int(rows['n_matches'][s])} {int(rows['n_seeds'][s])} {int(d['row_identity'][s:s + 1].view(np.uint32)[0])}")
    floats = tmp_path / "identities.txt"
    floats.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(floats)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) pairs, (\d+) anchors, (\d+) minimizers meeting several, (\d+) chains, (\d+) reversed chains, (\d+) ties met, (\d+) end ties, "
                 r"(\d+) band cuts that mattered, (\d+) trips above one, (\d+) tables, (\d+) fixture identities", r.stdout)
    assert m, r.stdout
    pairs, anchors, multi, chains, reversed_chains, ties, end_ties, band_cuts, trips, tables, identities = map(int, m.groups())
    print(r.stdout)
    assert pairs == 3 * 33648 + 6 * 360          # the multisets of 1 - 5 of 18 anchor types at three bands, the seeded pairs at six
    assert anchors > 0 and multi > 0 and chains > 0 and 0 < reversed_chains < chains
    assert ties > 0 and end_ties > 0 and band_cuts > 0 and trips > 0
    assert tables == 12 and identities == len(lines) > 3000
