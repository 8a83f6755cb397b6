"""metamdbg_amd/csrc/stitch_dev.hpp -- the word composition of mdbg_spans_stitch / mdbg_reads_stitch_ranges (a part of an oriented piece as
an oriented range of its read, its place at base d of a word in DnaBitset2's byte order, the invalid code under the flip; the ASCII form)
and the byte rule of mdbg_sequences_to_fasta_bytes -- compiled for the host with the address and undefined-behaviour sanitizers behind
serial copies of the lane loops of stitch_copy_kernel and fasta_write_kernel (tests/host/test_stitch.cpp), as a stand-alone program,
against a character-level model of CreateBaseContigsFunctor: pieces of 0 .. 70 bases joined at every offset mod 32, all four (read
window reversed) x (flip), mask bits at a piece's first and last base and just outside, each read's words in a heap block of exactly
its size; 40 one-base pieces in a row, empty pieces, contigs of 0 .. 4097 bases, a 70 000-base contig among 2 000 tiny ones; names of
every decimal width, all flags, an empty contig between two full ones."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_word_composition_owner_searches_and_text(tmp_path):
    exe = str(tmp_path / "test_stitch")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "test_stitch.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) contigs, (\d+) pieces, (\d+) output words, (\d+) words of more than two pieces, (\d+) words of 32 pieces, (\d+) pieces at a read's end, "
                 r"(\d+) masked pieces, (\d+) owners more than 64 on, (\d+) records, (\d+) bytes of text, (\d+) bytes touched outside the text", r.stdout)
    assert m, r.stdout
    contigs, pieces, words, over_two, of_32, at_end, masked, far, records, text_bytes, outside = map(int, m.groups())
    # (the program itself fails when an output word is not written exactly once, when padding is not zero, when a byte differs)
    # the sweep: 32 offsets x 71 lengths x 4 combinations x 2 mask states, each through both entries and both forms
    assert contigs >= 32 * 71 * 4 * 2 * 2 * 2
    assert pieces >= 3 * contigs // 2 and words >= 500_000
    assert over_two >= 1000                         # words that took more than two pieces ...
    assert of_32 >= 12                              # ... and the word of 32 one-base pieces: 2 mask states x 3 wave counts x 2 entries
    assert at_end >= 10_000                         # pieces that end at their read's last base (a heap block of exactly the read's words)
    assert masked == 32 * 70 * 4
    assert far >= 1000                              # the searches for the next contig and the next piece went well past their first steps
    assert records == 3 * (13 + 41 + 4) and text_bytes > 20_000
    assert outside == 0                             # no byte outside the text's n_bytes touched
