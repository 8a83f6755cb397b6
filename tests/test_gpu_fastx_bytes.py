"""mdbg_reads_from_fastx_bytes: FASTA / FASTQ text uploaded as it is and taken apart on the device.  The expected value is the text's
records by formats.fastx_records handed to mdbg_reads_from_ascii; the two read sets must be the same to every consumer: exported bases
and qualities, mdbg_reads_info, info[] and the scan's output (minimizers, positions, per-read arrays) with HPC on and off, which is what
proves the side masks and the masked list."""
from __future__ import annotations

import random

import numpy as np
import pytest

from metamdbg_amd import formats

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def scans(ctx, reads):
    out = []
    for hpc in (True, False):
        m = ctx.scan(reads, hpc=hpc)
        out.append(m.to_host())
        m.free()
    return out


def describe(ctx, reads, n):
    """Everything a consumer can see of a read set."""
    from metamdbg_amd import capi
    d = dict(info=reads.info(), scans=scans(ctx, reads))
    try:
        d["ascii"] = reads.export_ascii(0, n)
    except capi.MdbgError:                   # a batch with N bases exports read by read: all of a small one, a sample of a large one
        d["ascii"] = None                    # (the large tests compare every character on an N-free copy of their reads)
        step = max(1, n // 256)
        d["some"] = [reads.get(i) for i in range(0, n, step)]
    try:
        d["qual"] = reads.export_qualities(0, n)
    except capi.MdbgError:
        d["qual"] = None
    return d


def same(a, b):
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def expected(ctx, text):
    fmt, seqs, quals = formats.fastx_records(text)
    want = ctx.reads_from_ascii(seqs, quals)
    d = describe(ctx, want, len(seqs))
    want.free()
    n_masked = sum(1 for s in seqs if has_side_bits(s))
    d["fastx_info"] = dict(format=fmt, n_reads=len(seqs), n_bases=sum(map(len, seqs)), n_masked=n_masked)
    return d


def has_side_bits(s: bytes) -> bool:
    """A character with bit 3 set, or two neighbours that differ although their code and invalid bit agree (reads.hip)."""
    a = np.frombuffer(s, np.uint8)
    if (a & 8).any():
        return True
    return bool(len(a) > 1 and ((a[1:] != a[:-1]) & (((a[1:] ^ a[:-1]) & 0x0E) == 0)).any())


def check(ctx, text, want=None, begin=0, end=None, buffer=None):
    want = want or expected(ctx, text)
    b = ctx.bytes_from_host(buffer if buffer is not None else text)
    got = ctx.reads_from_fastx_bytes(b, begin, end)
    d = describe(ctx, got, want["fastx_info"]["n_reads"])
    d["fastx_info"] = got.fastx_info
    got.free()
    b.free()
    for k in want:
        assert same(d[k], want[k]), k
    return want


def fasta(seqs, width=None, eol=b"\n", last_eol=True, blank_every=0):
    out = []
    for i, s in enumerate(seqs):
        out.append(b">read_%d some description" % i + eol)
        w = width or max(1, len(s))
        for j, at in enumerate(range(0, len(s), w)):
            out.append(s[at:at + w] + eol)
            if blank_every and (i + j) % blank_every == 0:
                out.append(eol)
    text = b"".join(out)
    return text if last_eol else text[:-len(eol)]


def fastq(seqs, quals, eol=b"\n", last_eol=True):
    text = b"".join(b"@read_%d d" % i + eol + s + eol + b"+" + eol + q + eol for i, (s, q) in enumerate(zip(seqs, quals)))
    return text if last_eol else text[:-len(eol)]


LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129]


def plain_reads(rng, lengths):
    return [bytes(rng.choice(b"ACGT") for _ in range(L)) for L in lengths]


def odd_reads(rng):
    """N, runs of lower case, aA joins, an IUPAC letter; a change exactly at base 60 (a line join at width 60) and at base 32 / 64 (a
    word boundary)."""
    base = plain_reads(rng, [200] * 8)
    out = []
    for i, s in enumerate(base):
        s = bytearray(s)
        if i == 0: s[60:61] = b"N"
        if i == 1: s[59] = ord("A"); s[60:70] = b"a" + bytes(s[61:70]).lower()      # "Aa" across the join, then lower case
        if i == 2: s[31] = ord("a"); s[32] = ord("A")                               # "aA" across a word boundary
        if i == 3: s[63] = ord("C"); s[64] = ord("c")
        if i == 4: s[100:110] = b"NNNNNNNNNN"
        if i == 5: s[17] = ord("R"); s[18] = ord("Y")
        if i == 6: s[0] = ord("n"); s[199] = ord("N")
        out.append(bytes(s))
    return out


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
@pytest.mark.parametrize("width", [1, 60, 61, 64, None])
def test_fasta_small_shapes(ctx, width, eol):
    rng = random.Random(7)
    seqs = plain_reads(rng, LENGTHS) + odd_reads(rng) + plain_reads(rng, LENGTHS[::-1])
    want = None
    for last_eol in (True, False):
        for blank_every in (0, 3):
            want = check(ctx, fasta(seqs, width, eol, last_eol, blank_every), want)
    assert want["fastx_info"]["n_masked"] == 7 and want["info"]["n_reads"] == len(seqs)


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
def test_fastq_small_shapes(ctx, eol):
    rng = random.Random(8)
    seqs = plain_reads(rng, LENGTHS) + odd_reads(rng) + plain_reads(rng, [5, 300])
    quals = [bytes(rng.randrange(33, 127) for _ in s) for s in seqs]
    quals[-1] = b"@" + quals[-1][1:]              # quality lines that look like a header / a separator
    quals[-2] = b"+" + quals[-2][1:]
    quals[2] = b"@" * len(seqs[2])
    want = check(ctx, fastq(seqs, quals, eol))
    check(ctx, fastq(seqs, quals, eol, last_eol=False), want)
    check(ctx, fastq(seqs, quals, eol) + eol + eol, want)         # empty lines after the last record
    assert want["qual"] is not None and want["fastx_info"]["format"] == 1


def test_edge_cases(ctx):
    from metamdbg_amd import capi
    b = ctx.bytes_from_host(b">a\nACGT\n")
    r = ctx.reads_from_fastx_bytes(b, 3, 3)                       # an empty range
    assert r.info() == dict(n_reads=0, n_bases=0, n_words=0) and r.fastx_info["n_reads"] == 0
    check(ctx, b">only\nACGTTGCATTGACCA")                         # a single record without a trailing newline
    check(ctx, b"@only\nACGTTGCATTGACCA\n+\nIIIIIIIIIIIIIII")
    check(ctx, b">a\nA C\tG\n T\n>b\n\n\nAC GT\n")             # stripped white space
    check(ctx, b"@a\nA C\tG\n+\n12345\n@b\n\n+\n\n")              # ... whose qualities go with it; a read of length 0
    zero = b"".join(b">%d\n" % i for i in range(100_000))
    want = check(ctx, zero)
    assert want["info"] == dict(n_reads=100_000, n_bases=0, n_words=0)
    assert isinstance(ctx, capi.Context)


@pytest.mark.parametrize("text", [
    b"ACGT\n>a\nACGT\n",                       # a first byte that is neither marker
    b">a\nACGT\n+\nIIII\n",                    # FASTA with a '+' line
    b"@a\nAC\nGT\n+\nII\nII\n",                # multi-line FASTQ
    b"@a\nACGT\n+\nIII\n@b\nAC\n+\nII\n",      # a quality / sequence length mismatch
    b"@a\nACGT\n+\nIIII\n@b\nACGT\n",          # truncated after line 2 of a record
])
def test_refusals(ctx, text):
    from metamdbg_amd import capi
    with pytest.raises(ValueError):
        formats.fastx_records(text)
    b = ctx.bytes_from_host(text)
    with pytest.raises(capi.MdbgError) as ei:
        ctx.reads_from_fastx_bytes(b)
    assert ei.value.code == EINVAL and "mdbg_reads_from_fastx_bytes" in str(ei.value) and len(str(ei.value)) > 60
    check(ctx, b">a\nACGTACGTAC\n")            # the context is still usable


def many_reads(rng, n):
    """n reads of 200 - 3000 bases; one in sixteen soft-masked or with an N."""
    genome = np.frombuffer(bytes(rng.choice(b"ACGT") for _ in range(1 << 16)), np.uint8)
    seqs = []
    for i in range(n):
        L = rng.randrange(200, 3001)
        at = rng.randrange(0, len(genome) - L)
        s = genome[at:at + L].tobytes()
        if i % 16 == 5:
            cut = rng.randrange(0, L - 40)
            s = s[:cut] + s[cut:cut + 30].lower() + b"N" + s[cut + 31:]
        seqs.append(s)
    return seqs


def test_fasta_many_tiles(ctx):
    """One text of 8 - 16 MB: thousands of 16 KB tiles and every level of the scan, with records and line ends that straddle tile
    boundaries; a first header that grows by a byte 0 .. 15 times moves every boundary through a 16-byte load."""
    rng = random.Random(11)
    seqs = many_reads(rng, 6000)
    parts = [fasta(seqs[:2000], 60, b"\r\n", blank_every=0), fasta(seqs[2000:4000], None), fasta(seqs[4000:], 61, b"\n", blank_every=50)]
    body = b"".join(parts)
    assert 8 << 20 <= len(body) <= 16 << 20
    want = expected(ctx, body)
    assert want["info"]["n_reads"] == 6000 and want["fastx_info"]["n_masked"] == 375
    for grow in range(16):
        text = b">" + b"x" * grow + body[1:]
        if grow in (0, 7):
            assert formats.fastx_records(text)[1] == seqs
        check(ctx, text, want)


def no_side_bits(seqs):
    """The same reads in upper-case ACGT only: such a batch exports all its characters at once."""
    return [s.upper().replace(b"N", b"A") for s in seqs]


def test_every_character_of_the_large_texts(ctx):
    """The texts of the two many-tiles tests without N and lower case, so that export_ascii / export_qualities compare every base and
    every quality of every read, not a sample."""
    rng = random.Random(11)
    seqs = no_side_bits(many_reads(rng, 6000))
    text = b"".join([fasta(seqs[:2000], 60, b"\r\n"), fasta(seqs[2000:4000], None), fasta(seqs[4000:], 61, b"\n", blank_every=50)])
    want = check(ctx, text)
    assert want["ascii"] is not None and want["ascii"][0].tobytes() == b"".join(seqs)
    seqs = seqs[:2800]
    quals = [np.random.default_rng(i).integers(33, 127, len(s), dtype=np.uint8).tobytes() for i, s in enumerate(seqs)]
    want = check(ctx, fastq(seqs, quals, b"\r\n"))
    assert want["ascii"][0].tobytes() == b"".join(seqs) and want["qual"].tobytes() == b"".join(quals)


def test_lines_longer_than_a_tile(ctx):
    """Single-line reads of 40 - 100 kb: most 16 KB tiles hold no line start at all, so the class of the open line (FASTA) and the line
    index (FASTQ) are carried across whole tiles, and a tile's characters all lie in front of its first line start."""
    rng = random.Random(14)
    genome = np.random.default_rng(14).choice(np.frombuffer(b"ACGT", np.uint8), 1 << 18)
    seqs = []
    for L in (40_000, 100_000, 16_384, 1, 65_536 - 7, 0, 98_304):
        at = rng.randrange(0, len(genome) - L)
        seqs.append(genome[at:at + L].tobytes())
    for head in (b">", b">" + b"h" * 16_380, b">" + b"h" * 40_000):            # a header longer than a tile too
        text = head + fasta(seqs)[1:]
        want = check(ctx, text)
        assert want["ascii"][0].tobytes() == b"".join(seqs)
    masked = list(seqs)
    masked[1] = masked[1][:50_000] + b"acgtN" + masked[1][50_005:]
    check(ctx, fasta(masked, None, b"\r\n", last_eol=False))
    quals = [np.random.default_rng(i).integers(33, 127, len(s), dtype=np.uint8).tobytes() for i, s in enumerate(seqs)]
    for eol in (b"\n", b"\r\n"):
        want = check(ctx, fastq(seqs, quals, eol))
        assert want["ascii"][0].tobytes() == b"".join(seqs) and want["qual"].tobytes() == b"".join(quals)
    check(ctx, fastq(masked, quals, last_eol=False))


def test_fastq_many_tiles(ctx):
    rng = random.Random(12)
    seqs = many_reads(rng, 2800)
    quals = [np.random.default_rng(i).integers(33, 127, len(s), dtype=np.uint8).tobytes() for i, s in enumerate(seqs)]
    body = fastq(seqs, quals)
    assert len(body) >= 8 << 20
    want = expected(ctx, body)
    for grow in (0, 5, 11):
        check(ctx, b"@" + b"x" * grow + body[1:], want)


def test_range_inside_a_buffer(ctx):
    """begin at an offset that is no multiple of 16 and end before the buffer's: the bytes outside are poison that must not be read as
    records or line ends."""
    rng = random.Random(13)
    seqs = plain_reads(rng, [100, 0, 33, 5000, 64]) + odd_reads(rng)
    text = fasta(seqs, 60, last_eol=False)
    want = expected(ctx, text)
    for front in (b">\n>\n>", b"\n" * 37, b">p\nAC\n" * 700 + b">"):
        for back in (b">\n>\nACGT\n", b"\n>q\nAAAA\n" * 3000):
            buf = front + text + back
            assert len(front) % 16 != 0
            check(ctx, text, want, begin=len(front), end=len(front) + len(text), buffer=buf)
    quals = [bytes(rng.randrange(33, 127) for _ in s) for s in seqs]
    text = fastq(seqs, quals, last_eol=False)
    want = expected(ctx, text)
    buf = b"@\n@\n+" + text + b"\n@x\nAC\n+\nII\n"
    check(ctx, text, want, begin=5, end=5 + len(text), buffer=buf)
