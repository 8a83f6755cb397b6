"""mdbg_bytes_inflate_bgzf / mdbg_bytes_download / mdbg_fastx_whole_records: BGZF blocks inflated on the device.  zlib in Python is the
expected value; the text is read back with download.  The corpus is the one tests/host/test_deflate_core.cpp puts through the decoder's
core on the host (every zlib level and strategy, DNA, FASTQ, runs, periodic text, far matches, stored blocks, tiny inputs, flushed
streams, a hand-made dynamic block); the refusals are of the kinds it checks there first, and the very bytes sent to the device are
put before zlib here, which must refuse block 2 and accept the others."""
from __future__ import annotations

import random
import struct
import zlib

import numpy as np
import pytest

from metamdbg_amd import formats

pytestmark = pytest.mark.gpu

EINVAL = -1
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def wrap(payload: bytes, data: bytes) -> bytes:
    """A BGZF member around a raw DEFLATE payload made by hand."""
    bsize = 18 + len(payload) + 8
    assert bsize <= 65536
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1) + payload
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def inflate(ctx, comp_raw, blocks, text_at=0, room=None):
    """The blocks inflated behind text_at of a buffer filled with 0xA5; returns (text, whole buffer)."""
    total = sum(b[2] for b in blocks)
    size = text_at + total + GUARD if room is None else room
    comp = ctx.bytes_from_host(comp_raw if comp_raw else b"\0")
    text = ctx.bytes_from_host(b"\xA5" * size)
    try:
        n = ctx.inflate_bgzf(comp, blocks, text, text_at)
        assert n == total
        whole = text.download(0, size)
    finally:
        comp.free()
        text.free()
    assert whole[:text_at] == b"\xA5" * text_at, "bytes in front of the range were written"
    assert whole[text_at + total:] == b"\xA5" * (size - text_at - total), "bytes behind the range were written"
    return whole[text_at:text_at + total], whole


def check_file(ctx, raw, data, text_at=0):
    blocks = formats.bgzf_blocks(raw)
    assert blocks is not None
    got, _ = inflate(ctx, raw, blocks, text_at)
    assert got == data
    return blocks


# ---- the corpus ----------------------------------------------------------------------------------------------------------------------
def dna(rng, n, line=0):
    s = bytes(rng.choice(b"ACGT") for _ in range(n))
    if line:
        s = b"\n".join(s[i:i + line] for i in range(0, n, line))[:n]
    return s


def fastq_text(rng, n):
    out, i = [], 0
    while sum(map(len, out)) < n:
        L = rng.randrange(50, 450)
        out.append(b"@read%d\n" % i + bytes(rng.choice(b"ACGT") for _ in range(L)) + b"\n+\n" + bytes(rng.randrange(33, 81) for _ in range(L)) + b"\n")
        i += 1
    return b"".join(out)[:n]


def periodic(rng, p, n):
    unit = bytes(rng.randrange(256) for _ in range(p))
    return (unit * (n // p + 1))[:n]


class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, k):
        for i in range(k):
            self.acc |= ((v >> i) & 1) << self.n
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                self.acc, self.n = 0, 0

    def code(self, c, length):                                  # Huffman codes go most significant bit first
        for i in range(length):
            self.bits((c >> (length - 1 - i)) & 1, 1)

    def done(self):
        if self.n:
            self.out.append(self.acc)
        return bytes(self.out)


def handmade_dynamic():
    """A dynamic block whose distance code has ONE symbol of length 1 (incomplete, accepted by zlib): 'A' 'C' and two matches."""
    w = Bits()
    w.bits(1, 1); w.bits(2, 2)
    w.bits(1, 5); w.bits(0, 5); w.bits(14, 4)                   # HLIT 258, HDIST 1, HCLEN 18
    for s in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1]:
        w.bits(2 if s in (0, 1, 2, 18) else 0, 3)               # code-length code: 0 -> 00, 1 -> 01, 2 -> 10, 18 -> 11

    def zeros(n):
        w.code(3, 2); w.bits(n - 11, 7)
    zeros(65); w.code(2, 2); w.code(0, 2); w.code(2, 2)
    zeros(138); zeros(50)
    w.code(2, 2); w.code(2, 2)
    w.code(1, 2)                                                # the distance code's only entry: length 1
    # literal/length codes: 'A' 00, 'C' 01, end-of-block 10, length 3 11
    w.code(0, 2); w.code(1, 2); w.code(3, 2); w.code(0, 1); w.code(0, 2); w.code(3, 2); w.code(0, 1); w.code(2, 2)
    payload, data = w.done(), b"ACCCCAAAA"
    assert zlib.decompress(payload, -15) == data
    return payload, data


def flushed(data, every, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    out = []
    for at in range(0, len(data), every):
        out.append(c.compress(data[at:at + every]))
        out.append(c.flush(zlib.Z_FULL_FLUSH))
    out.append(c.flush())
    return b"".join(out)


def corpus():
    """[(name, BGZF member, text)]: every item is one block."""
    rng = random.Random(1951)
    items = []
    mixed = fastq_text(rng, 20000) + dna(rng, 12000, 80)
    for level in (0, 1, 6, 9):
        for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE):
            items.append((f"level {level} strategy {strategy}", formats.bgzf_member(mixed, level, strategy), mixed))
    for name, d in [("dna one line", dna(rng, 60000)), ("dna 60 columns", dna(rng, 60000, 60)), ("fastq 33-80", fastq_text(rng, 65000)),
                    ("65280 of one byte", b"A" * 65280), ("65536 of one byte", b"T" * 65536),
                    ("random (stored)", bytes(rng.randrange(256) for _ in range(65000))),
                    ("empty", b""), ("one byte", b"x"), ("two bytes", b"xy")]:
        items.append((name, formats.bgzf_member(d), d))
    for p in (1, 2, 3, 4, 63, 64, 65, 257, 258, 259):
        d = periodic(rng, p, 20000 + p)
        items.append((f"period {p}", formats.bgzf_member(d), d))
    far = bytes(rng.randrange(256) for _ in range(40 * 1024))
    far += far[:300]
    items.append(("far match", formats.bgzf_member(far, 9), far))
    d = fastq_text(rng, 30000)
    items.append(("full flush every 1000", wrap(flushed(d, 1000), d), d))
    payload, d = handmade_dynamic()
    items.append(("one distance code", wrap(payload, d), d))
    return items


CORPUS = corpus()


@pytest.mark.parametrize("name,raw,data", CORPUS, ids=[c[0] for c in CORPUS])
def test_corpus_one_block(ctx, name, raw, data):
    check_file(ctx, raw, data)


@pytest.fixture(scope="module")
def text_200k():
    return fastq_text(random.Random(7), 200000)


@pytest.mark.parametrize("block", [1, 2, 3000, 0xFF00, 65536])
def test_block_sizes(ctx, text_200k, block):
    data = text_200k[:300] if block < 3 else text_200k
    check_file(ctx, formats.bgzf_compress(data, block=block), data)


def test_block_counts_and_the_grid_stride_loop(ctx, text_200k):
    chunks = [text_200k[i * 3000:(i + 1) * 3000] for i in range(16)]
    members = [formats.bgzf_member(c, 1 + i % 9) for i, c in enumerate(chunks)]
    empty = formats.bgzf_member(b"")
    n_cu = ctx.device_info()["n_cu"]
    for count in (1, 2, 63, 64, 65, 8 * n_cu * 4 + 3):
        raw, data = [], []
        for i in range(count):
            raw.append(members[i % 16]); data.append(chunks[i % 16])
            if i % 29 == 7:
                raw.append(empty)                              # empty blocks in the middle
        raw.append(empty)                                      # and the EOF marker
        blocks = check_file(ctx, b"".join(raw), b"".join(data))
        assert len(blocks) == count + 1 + len([i for i in range(count) if i % 29 == 7])
    assert inflate(ctx, b"", [])[0] == b""                     # n_blocks == 0


@pytest.mark.parametrize("text_at", [0, 1, 3, 17, 4097])
def test_text_at_and_guards(ctx, text_200k, text_at):
    data = text_200k[:70001]
    check_file(ctx, formats.bgzf_compress(data, block=9973), data, text_at=text_at)


def test_payloads_at_odd_offsets(ctx, text_200k):
    data = text_200k[:40000]
    raw = formats.bgzf_compress(data, block=2999)
    blocks = formats.bgzf_blocks(raw)
    seen = set()
    for shift in (0, 1, 2, 3):
        moved = [(src + shift, csize, isize, crc) for src, csize, isize, crc in blocks]
        seen |= {src & 3 for src, _, _, _ in moved}
        got, _ = inflate(ctx, b"\xEE" * shift + raw, moved)
        assert got == data
    assert seen == {0, 1, 2, 3}


# ---- refusals: checked inputs, not faults --------------------------------------------------------------------------------------------
def refusal_cases(data):
    raw = formats.bgzf_compress(data, block=3000, level=6)
    good = formats.bgzf_blocks(raw)
    i = 2
    src, csize, isize, crc = good[i]

    def table(entry):
        return good[:i] + [entry] + good[i + 1:]
    cases = [("a flipped CRC", raw, table((src, csize, isize, crc ^ 1)), "CRC-32 mismatch"),
             ("isize one too large", raw, table((src, csize, isize + 1, crc)), "block 2"),
             ("isize one too small", raw, table((src, csize, isize - 1, crc)), "block 2"),
             ("csize one short", raw, table((src, csize - 1, isize, crc)), "block 2"),
             ("src + csize beyond the buffer", raw, table((len(raw) - 10, 11, isize, crc)), "block 2")]
    bad = bytearray(raw)
    bad[src] |= 6
    cases.append(("block type 3", bytes(bad), good, "reserved block type"))
    stored = formats.bgzf_compress(data, block=3000, level=0)
    sb = formats.bgzf_blocks(stored)
    bad = bytearray(stored)
    bad[sb[i][0] + 3] ^= 0x10                                  # NLEN of the block's first (only) stored block
    cases.append(("a stored block with a wrong NLEN", bytes(bad), sb, "stored LEN/NLEN mismatch"))
    return raw, good, cases


def zlib_accepts(comp_raw, block):
    """zlib's verdict on one table entry: the payload is a complete raw DEFLATE stream of exactly isize bytes with this CRC-32."""
    src, csize, isize, crc = block
    if src + csize > len(comp_raw):
        return False
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(comp_raw[src:src + csize])
    except zlib.error:
        return False
    return d.eof and len(out) == isize and zlib.crc32(out) & 0xFFFFFFFF == crc


def test_refusals_and_the_call_after_them(ctx, text_200k):
    from metamdbg_amd import capi
    data = text_200k[:20000]
    raw, good, cases = refusal_cases(data)
    for name, comp_raw, blocks, needle in cases:
        # the very bytes sent to the device are bad by zlib's account too, in block 2 and nowhere else
        assert [zlib_accepts(comp_raw, b) for b in blocks] == [i != 2 for i in range(len(blocks))], name
        with pytest.raises(capi.MdbgError) as e:
            inflate(ctx, comp_raw, blocks, room=len(data) + 2 * GUARD)
        assert e.value.code == EINVAL, name
        assert "block 2" in str(e.value) and needle in str(e.value), (name, str(e.value))
        assert inflate(ctx, raw, good)[0] == data, name        # the same context goes on working
    with pytest.raises(capi.MdbgError) as e:                   # a total too large for the text
        inflate(ctx, raw, good, text_at=5, room=5 + len(data) - 1)
    assert e.value.code == EINVAL and f"block {len(good) - 2}" in str(e.value), str(e.value)
    with pytest.raises(capi.MdbgError) as e:
        inflate(ctx, raw, good[:1] + [(good[1][0], good[1][1], 65537, 0)], room=1 << 17)
    assert e.value.code == EINVAL and "block 1" in str(e.value)
    with pytest.raises(capi.MdbgError) as e:                   # a payload longer than a BGZF member, inside the buffer
        inflate(ctx, raw + bytes(70000), good[:1] + [(good[1][0], 65537, good[1][2], good[1][3])])
    assert e.value.code == EINVAL and "block 1" in str(e.value) and "csize" in str(e.value)
    assert inflate(ctx, raw, good)[0] == data


def test_download_checks_its_range(ctx):
    from metamdbg_amd import capi
    b = ctx.bytes_from_host(b"0123456789")
    assert b.download(3, 4) == b"3456" and b.download(10, 0) == b"" and b.download(0, 10) == b"0123456789"
    for at, n in ((0, 11), (11, 0), (5, 6)):
        with pytest.raises(capi.MdbgError) as e:
            b.download(at, n)
        assert e.value.code == EINVAL
    b.free()


# ---- inflate, then parse: the same read set as the text uploaded plain ---------------------------------------------------------------
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
    except capi.MdbgError:
        d["ascii"] = None
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


LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129]


def read_texts():
    rng = random.Random(11)
    lens = [LENGTHS[i % len(LENGTHS)] if i % 40 else 3000 for i in range(200)]
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(L)) for L in lens]
    quals = [bytes(rng.randrange(33, 81) for _ in range(L)) for L in lens]
    fa = b"".join(b">read_%d d\r\n" % i + b"".join(s[at:at + 70] + b"\r\n" for at in range(0, len(s), 70)) for i, s in enumerate(seqs))
    fq = b"".join(b"@read_%d d\n" % i + s + b"\n+\n" + q + b"\n" for i, (s, q) in enumerate(zip(seqs, quals)))
    return [("fasta", fa), ("fastq", fq)]


@pytest.mark.parametrize("name,text", read_texts(), ids=["fasta", "fastq"])
def test_inflated_text_parses_like_plain_text(ctx, name, text):
    plain = ctx.bytes_from_host(text)
    r = ctx.reads_from_fastx_bytes(plain)
    n = r.fastx_info["n_reads"]
    assert n == 200
    want = describe(ctx, r, n)
    want["fastx_info"] = r.fastx_info
    r.free(); plain.free()
    raw = formats.bgzf_compress(text, block=3000)
    comp = ctx.bytes_from_host(raw)
    buf = ctx.bytes_create(len(text))
    assert ctx.inflate_bgzf(comp, formats.bgzf_blocks(raw), buf) == len(text)
    r = ctx.reads_from_fastx_bytes(buf)                        # no synchronisation in between
    got = describe(ctx, r, n)
    got["fastx_info"] = r.fastx_info
    r.free(); buf.free(); comp.free()
    for k in want:
        assert same(got[k], want[k]), k


# ---- where the last whole record ends ------------------------------------------------------------------------------------------------
def whole_records_rule(text, begin, end):
    if text[begin:begin + 1] == b">":
        p = text.rfind(b"\n>", begin, end)
        return (p + 1 if p >= 0 else begin), 0
    nl = [i for i in range(begin, end) if text[i] == 10]
    k = len(nl) // 4 * 4
    return (nl[k - 1] + 1 if k else begin), 1


def check_cuts(ctx, text, begin, ends):
    b = ctx.bytes_from_host(text)
    try:
        for end in ends:
            assert ctx.fastx_whole_records(b, begin, end) == whole_records_rule(text, begin, end), (begin, end)
    finally:
        b.free()


FA3 = b">r0 x\nACGT\nAC\n>r1\n\n>r2 > y\nGG>A\n>\n"
FQ3 = b"@r0\nACGT\n+\n@>II\n@r1\nAC\n+r1\n>@\n@r2\nA\n+\n@\n"      # quality lines that start with '@' and with '>'


@pytest.mark.parametrize("text", [FA3, FQ3], ids=["fasta", "fastq"])
def test_whole_records_at_every_offset(ctx, text):
    from metamdbg_amd import capi
    check_cuts(ctx, text, 0, range(1, len(text) + 1))
    second = text.index(b"\n>r1" if text[:1] == b">" else b"\n@r1") + 1
    check_cuts(ctx, text, second, range(second + 1, len(text) + 1))
    b = ctx.bytes_from_host(text)
    for begin, end in ((1, len(text)), (0, 0), (0, len(text) + 1)):      # not a record start; empty; outside
        with pytest.raises(capi.MdbgError) as e:
            ctx.fastx_whole_records(b, begin, end)
        assert e.value.code == EINVAL
    b.free()


@pytest.mark.parametrize("fq", [False, True], ids=["fasta", "fastq"])
def test_whole_records_at_tile_borders(ctx, fq):
    rng = random.Random(3)
    recs = []
    while sum(map(len, recs)) < 40 * 16384:
        L = rng.randrange(1, 900)
        s = bytes(rng.choice(b"ACGT") for _ in range(L))
        recs.append(b"@r\n" + s + b"\n+\n" + b">" * L + b"\n" if fq else b">r\n" + s + b"\n")
    text = b"".join(recs)[:40 * 16384]
    ends = [t * 16384 + d for t in range(1, 41) for d in (-1, 0, 1) if t * 16384 + d <= len(text)]
    check_cuts(ctx, text, 0, ends)
    begin = len(recs[0])                                       # an unaligned begin moves nothing
    check_cuts(ctx, text, begin, ends[::7])
