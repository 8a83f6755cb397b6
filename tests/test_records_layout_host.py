"""metamdbg_amd/csrc/records_dev.hpp -- the layout of the two record forms and the composition of their bytes from aligned words and
single bytes that records_write_kernel runs -- compiled for the host with the address and undefined-behaviour sanitizers
(tests/host/test_records_layout.cpp) and run in a serial copy of the kernel's lane loop: every byte of a buffer of exactly n_bytes is
stored exactly once, a word store never crosses a section or a record, and the result is the field-by-field serialisation, for every
count 0 .. 70 at every alignment of the record's start, for zero records, one record, a record of 70 001 values and seeded random
sets; the offset arithmetic also behind more than 2^32 minimizers."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_composition_against_field_by_field_serialisation(tmp_path):
    exe = str(tmp_path / "test_records_layout")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "test_records_layout.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) sets, (\d+) records, (\d+) bytes, (\d+) word stores, (\d+) byte stores, (\d+) count-residue pairs, (\d+) records behind 2\^32 minimizers", r.stdout)
    assert m, r.stdout
    sets, records, n_bytes, words, single, pairs, far = map(int, m.groups())
    assert sets >= 100 and records >= 10_000 and n_bytes >= 1_000_000
    assert pairs == 2 * 71 * 4                      # both forms, counts 0 .. 70, four residues: the program fails if one did not occur
    assert words > 0 and single > 0
    assert 4 * words + single == n_bytes            # every byte stored once, by a word or alone
    assert 4 * words > n_bytes // 2                 # ... and most of them in words
    assert far >= 100
