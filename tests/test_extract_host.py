"""metamdbg_amd/csrc/extract_dev.hpp -- the word composition of mdbg_spans_extract / mdbg_reads_extract_ranges (the gather of up to 32
bases from two source words, the code exchange, the complement, the invalid mask, the tail, the group reversal inside bytes or the byte
swap; the ASCII form; the range of a (window, part) request) -- compiled for the host with the address and undefined-behaviour sanitizers
behind a serial copy of extract_copy_kernel's lane loop (tests/host/test_extract.cpp), against a character-level model of memcpy +
Utils::revcomp + DnaBitset2: every start 0 .. 63 x every length 0 .. 130 x both orientations x both forms, with and without an invalid mask
whose bits sit at the range's first and last base and just outside it, ranges that end at their read's last base (each read's words in a
heap block of exactly its size), batches over reads packed back to back with lengths 0 and 70 000 and stretches of tiny ranges (the
search for a lane's next owner, extract_next_owner); every output word written once, padding
zero, nothing of a neighbouring read used."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_word_composition_offsets_and_parts(tmp_path):
    exe = str(tmp_path / "test_extract")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "test_extract.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) ranges, (\d+) output words, (\d+) masked reads, (\d+) ranges at a read's end, (\d+) with a second source word, (\d+) batches, "
                 r"(\d+) parts, (\d+) owners more than 64 requests on", r.stdout)
    assert m, r.stdout
    ranges, words, masked, at_end, two_words, batches, parts, far_owners = map(int, m.groups())
    # the sweep: 64 starts x 131 lengths x 2 tails x 2 mask states, less the one empty read of each mask state, x 2 orientations x 2 forms
    assert ranges >= (64 * 131 * 2 * 2 - 2) * 4
    assert words >= 500_000
    assert masked == 64 * 131 * 2 - 1 and at_end >= 64 * 131 * 2 - 2
    assert two_words >= 20_000                      # the gather took its second source word
    assert batches == 6 and parts == 60_000
    assert far_owners >= 100                        # the search for the next owner went well past its first steps
