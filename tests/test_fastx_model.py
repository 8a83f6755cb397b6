"""formats.fastx_records -- the plain-Python statement of the record rules of mdbg_reads_from_fastx_bytes -- against hand-written
expectations (one per rule, every refusal), the tiny FASTA / FASTQ inputs under tests/golden, and seeded well-formed files."""
from __future__ import annotations

import os
import random

import pytest

from metamdbg_amd import formats
from tests import helpers

F = formats.fastx_records


@pytest.mark.parametrize("text, want", [
    (b"", (0, [], None)),                                                   # an empty range: zero reads
    (b">a\nACGT\n", (0, [b"ACGT"], None)),
    (b">a desc > @ +\nACGT\n", (0, [b"ACGT"], None)),                       # the header line is skipped whatever it holds
    (b">a\nAC\nGT\nTT\n>b\nA\n", (0, [b"ACGTTT", b"A"], None)),             # multi-line
    (b">a\r\nAC\r\nGT\r\n>b\r\nA\r\n", (0, [b"ACGT", b"A"], None)),         # CR-LF
    (b">a\nAC\n\n\nGT\n\n>b\n\nA\n", (0, [b"ACGT", b"A"], None)),           # blank lines
    (b">a\nAC\nGT", (0, [b"ACGT"], None)),                                  # a last line without a newline
    (b">a\nA C\tG\n T\n", (0, [b"ACGT"], None)),                            # space and tab are stripped
    (b">a\n>b\nAC\n>c\n", (0, [b"", b"AC", b""], None)),                    # a header after a header: a read of length 0
    (b">a", (0, [b""], None)),
    (b">a\nAC>GT@+\n", (0, [b"AC>GT@+"], None)),                            # markers count at a line's first byte only
    (b"@a\nACGT\n+\nIIII\n", (1, [b"ACGT"], [b"IIII"])),
    (b"@a\nACGT\n+a\nIIII", (1, [b"ACGT"], [b"IIII"])),                     # no trailing newline
    (b"@a\r\nACGT\r\n+\r\nIIII\r\n", (1, [b"ACGT"], [b"IIII"])),            # a trailing \r is dropped from both
    (b"@a\nACGT\n+\n@III\n@b\nAC\n+\n+I\n", (1, [b"ACGT", b"AC"], [b"@III", b"+I"])),   # quality lines that start with a marker
    (b"@a\nACGT\n+\nIIII\n\n\r\n\n", (1, [b"ACGT"], [b"IIII"])),            # empty lines after the last record
    (b"@a\n\n+\n\n@b\nA\n+\nI\n", (1, [b"", b"A"], [b"", b"I"])),           # a read of length 0
    (b"@a\n\n+\n", (1, [b""], [b""])),                                      # ... whose empty quality line is not there
    (b"@a\nA C\tG\n+\n12345\n", (1, [b"ACG"], [b"135"])),                   # a stripped base takes its quality with it
    (b"@a\nACG\n+\n! ~\n", (1, [b"ACG"], [b"! ~"])),                       # quality bytes pass through unchanged
])
def test_each_rule(text, want):
    assert F(text) == want


@pytest.mark.parametrize("text, where", [
    (b"ACGT\n", "begin"),                              # neither marker
    (b"\n>a\nACGT\n", "begin"),
    (b">a\nAC\n+\nII\n", "line 3"),                    # FASTA with a '+' line: kseq would read qualities
    (b">a\nAC\n@b\nAC\n", "line 3"),                   # ... with an '@' line
    (b"@a\nAC\nGT\n+\nII\nII\n", "line 3"),            # multi-line FASTQ
    (b"@a\nACGT\n+\nIII\n", "line 4"),                 # fewer qualities than bases
    (b"@a\nACG\n+\nIIII\n", "line 4"),                 # more
    (b"@a\nACGT\n", "line 3"),                         # truncated after line 2
    (b"@a\nACGT\n+\n", "line 4"),                      # truncated after line 3
    (b"@a\nACGT\n+\nIIII\nb\nAC\n+\nII\n", "line 5"),  # the second record does not start with '@'
    (b"@a\nACGT\n+\nIIII\n\n@b\nAC\n+\nII\n", "line 5"),   # an empty line between records moves the count
])
def test_each_refusal(text, where):
    with pytest.raises(ValueError, match=where):
        F(text)


def test_golden_inputs():
    fa = os.path.join(helpers.GOLDEN, "edge", "edge.fasta")
    fq = os.path.join(helpers.GOLDEN, "edge", "edge.fastq")
    assert F(open(fa, "rb").read()) == (0, helpers.read_fasta(fa), None)
    seqs, quals = helpers.read_fastq(fq)
    assert F(open(fq, "rb").read()) == (1, seqs, quals)


def random_fastx(rng: random.Random, fastq: bool, n: int, max_len: int = 300):
    """(text, seqs, quals): a well-formed file with random line widths, line ends, blank lines and soft-masked / N stretches."""
    eol = rng.choice([b"\n", b"\r\n"])
    seqs, quals, out = [], [], []
    for i in range(n):
        L = rng.choice([0, 1, rng.randrange(max_len), rng.randrange(max_len)])
        s = bytes(rng.choice(b"ACGTACGTACGTacgtNnRY") for _ in range(L))
        seqs.append(s)
        if fastq:
            q = bytes(rng.randrange(33, 127) for _ in range(L))
            quals.append(q)
            out += [b"@r%d x" % i, eol, s, eol, b"+", eol, q, eol]
        else:
            out += [b">r%d x" % i, eol]
            w = rng.choice([1, 7, 60, 61, 64, max_len + 1])
            for at in range(0, L, w):
                out += [s[at:at + w], eol]
                if rng.random() < 0.05:
                    out.append(eol)
    text = b"".join(out)
    if rng.random() < 0.5 and text.endswith(eol) and (not fastq or seqs[-1]):
        text = text[:-len(eol)]
    return text, seqs, (quals if fastq else None)


@pytest.mark.parametrize("fastq", [False, True])
def test_seeded_random_files(fastq):
    rng = random.Random(20240 + fastq)
    for _ in range(40):
        text, seqs, quals = random_fastx(rng, fastq, rng.randrange(1, 40))
        assert F(text) == (int(fastq), seqs, quals)
