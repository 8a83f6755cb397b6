"""mdbg_bytes_inflate_gzip / mdbg_bytes_copy: ordinary gzip (one deflate stream per member, no index) inflated on the device in chunks
that start at deflate block headers.  zlib in Python is the expected text; the chunk starts come from formats.deflate_block_starts.
Texts are 300 - 400 KB in 3 to 12 chunks: the smallest at which windows span chunks, members end inside chunks and a chunk overflows its
first capacity.  The refusals are inputs zlib refuses too (or, for a wrong start, that no decoder could take)."""
from __future__ import annotations

import random
import struct
import zlib

import numpy as np
import pytest

from metamdbg_amd import formats

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -1, -5
GUARD = 64
TO_END = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


# ---- gzip files and their block headers ----------------------------------------------------------------------------------------------
def member(data: bytes, level: int = 6, strategy: int = 0, sync_at=(), flags: int = 0) -> bytes:
    """A gzip member; ``sync_at``: text offsets behind which the compressor is flushed (Z_SYNC_FLUSH: a byte-aligned start that keeps
    history); ``flags``: FEXTRA 4 | FNAME 8 | FCOMMENT 16 | FHCRC 2."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    out, at = [], 0
    for cut in sync_at:
        out.append(c.compress(data[at:cut])); out.append(c.flush(zlib.Z_SYNC_FLUSH))
        at = cut
    out.append(c.compress(data[at:])); out.append(c.flush())
    return wrap(b"".join(out), data, flags)


def wrap(payload: bytes, data: bytes, flags: int = 0, crc=None, isize=None) -> bytes:
    head = b"\x1f\x8b\x08" + bytes([flags]) + b"\0\0\0\0\0\x03"
    if flags & 4:
        extra = bytes(range(256)) * 3
        head += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        head += b"reads.fastq\0"
    if flags & 16:
        head += b"a comment " * 40 + b"\0"
    if flags & 2:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return (head + payload + struct.pack("<II", (zlib.crc32(data) if crc is None else crc) & 0xFFFFFFFF, (len(data) if isize is None else isize) & 0xFFFFFFFF))


def header_size(raw: bytes, at: int) -> int:
    assert raw[at:at + 3] == b"\x1f\x8b\x08"
    flags, p = raw[at + 3], at + 10
    if flags & 4:
        p += 2 + struct.unpack_from("<H", raw, p)[0]
    if flags & 8:
        p = raw.index(b"\0", p) + 1
    if flags & 16:
        p = raw.index(b"\0", p) + 1
    if flags & 2:
        p += 2
    return p - at


def file_blocks(raw: bytes):
    """([(bit of a block header, text in front of it, member)], [(header byte, first block bit, byte behind the trailer)] per member)"""
    blocks, members, at, text = [], [], 0, 0
    while raw[at:at + 2] == b"\x1f\x8b":
        first = (at + header_size(raw, at)) * 8
        bl, end = formats.deflate_block_starts(raw, first)
        blocks += [(bit, text + before, len(members)) for bit, _, _, before in bl]
        behind = (end + 7) // 8 + 8
        text += struct.unpack_from("<I", raw, behind - 4)[0]
        members.append((at, first, behind))
        at = behind
    return blocks, members


def dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def fasta_text(rng, n):
    out, i = [], 0
    while sum(map(len, out)) < n:
        s = dna(rng, rng.randrange(2000, 11000))
        out.append(b">read_%d ccs\n" % i + b"\n".join(s[a:a + 80] for a in range(0, len(s), 80)) + b"\n")
        i += 1
    return b"".join(out)[:n]


def fastq_text(rng, n):
    out, i = [], 0
    while sum(map(len, out)) < n:
        L = rng.randrange(500, 5500)
        out.append(b"@read_%d\n" % i + dna(rng, L) + b"\n+\n" + bytes(rng.randrange(33, 81) for _ in range(L)) + b"\n")
        i += 1
    return b"".join(out)[:n]


_cache: dict = {}


def texts():
    if "texts" not in _cache:
        rng = random.Random(1952)
        _cache["texts"] = (fasta_text(rng, 310000), fastq_text(rng, 330000))
    return _cache["texts"]


def make_item(name: str):
    fa, fq = texts()
    a, b, c = fa[:120000], fq[:110000], fa[120000:250000]
    if name.startswith("fasta level"):
        return member(fa, int(name[-1])), fa
    if name.startswith("fastq level"):
        return member(fq, int(name[-1])), fq
    if name == "stored only":
        return member(fq, 0), fq
    if name == "fixed Huffman":
        return member(fa, 6, zlib.Z_FIXED, sync_at=(100000, 200000)), fa
    if name == "sync flush points":
        return member(fq, 6, sync_at=(100000, 110000, 250000)), fq       # 10 000 bytes of text between two starts: a window spans two chunks
    if name == "three members":
        return member(a, 6, sync_at=(40000, 80000)) + member(b, 1, sync_at=(50000,)) + member(c, 9, sync_at=(40000, 80000)), a + b + c      # (flushed: every member has several blocks)
    if name == "an empty member in the middle":
        return member(a, 6, sync_at=(40000, 80000)) + member(b"", 6) + member(b, 6, sync_at=(50000,)), a + b
    if name == "header fields":
        return member(a, 6, flags=2) + member(b, 6, flags=4 | 8 | 16 | 2), a + b
    if name == "trailing garbage":
        return member(fa[60000:], 6) + bytes(random.Random(5).randrange(1, 256) for _ in range(300)), fa[60000:]
    if name == "a run":
        d = b"A" * 600000
        return member(d, 9), d
    raise KeyError(name)


def item(name: str):
    """(file, text, blocks, members), made once"""
    if name not in _cache:
        raw, data = make_item(name)
        blocks, members = file_blocks(raw)
        _cache[name] = (raw, data, blocks, members)
    return _cache[name]


ITEMS = ["fasta level 1", "fasta level 6", "fasta level 9", "fastq level 1", "fastq level 6", "fastq level 9", "stored only", "fixed Huffman", "sync flush points",
         "three members", "an empty member in the middle", "header fields", "trailing garbage"]


def chunks_of(starts, first=0, last=TO_END):
    edges = [first] + list(starts) + [last]
    return [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]


def inflate(ctx, raw, chunks, want_len, text_at=0, room=None, stream=None):
    """One call on ``stream`` (a fresh one by default) into a buffer filled with 0xA5; returns (text, info)."""
    size = text_at + want_len + GUARD if room is None else room
    comp = ctx.bytes_from_host(raw)
    text = ctx.bytes_from_host(b"\xA5" * size)
    own = stream is None
    if own:
        stream = ctx.gzip_stream()
    try:
        info = ctx.inflate_gzip(stream, comp, chunks, text, text_at)
        whole = text.download(0, size)
    finally:
        comp.free()
        text.free()
        if own:
            stream.free()
    n = info["n_text"]
    assert whole[:text_at] == b"\xA5" * text_at, "bytes in front of the range were written"
    assert whole[text_at + n:] == b"\xA5" * (size - text_at - n), "bytes behind the range were written"
    return whole[text_at:text_at + n], info


def inner_starts(blocks):
    return [bit for bit, _, _ in blocks[1:]]


# ---- the corpus, whole and cut at every block ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ITEMS)
def test_corpus_whole_and_cut_at_every_block(ctx, name):
    raw, data, blocks, members = item(name)
    got, info = inflate(ctx, raw, chunks_of([]), len(data))
    assert got == data
    assert info == dict(n_text=len(data), members=len(members), ended=1, end_bit=members[-1][2] * 8)
    starts = inner_starts(blocks)
    assert 2 <= len(starts) <= 40, len(starts)
    got, info = inflate(ctx, raw, chunks_of(starts), len(data))
    assert got == data
    assert info == dict(n_text=len(data), members=len(members), ended=1, end_bit=members[-1][2] * 8)


def test_a_window_that_spans_two_chunks(ctx):
    raw, data, blocks, _ = item("sync flush points")
    by_text = {}
    for bit, before, _ in blocks:
        by_text.setdefault(before, bit)
    starts = [by_text[100000], by_text[110000]]                # the chunk between them holds 10 000 bytes: the last chunk's window reaches over it
    got, _ = inflate(ctx, raw, chunks_of(starts), len(data))
    assert got == data


# ---- distances zlib's deflate never emits: a hand-made fixed-Huffman stream -----------------------------------------------------------------
class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, k):
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, length):                                  # Huffman codes go most significant bit first
        self.bits(int(format(c, "0%db" % length)[::-1], 2), length)

    def literal(self, b):
        if b < 144:
            self.code(0x30 + b, 8)
        else:
            self.code(0x190 + b - 144, 9)

    def length_symbol(self, s):                                 # 256 .. 287
        if s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def position(self):
        return len(self.out) * 8 + self.n

    def done(self):
        if self.n:
            self.out.append(self.acc)
        return bytes(self.out)


def far_match_stream(dist):
    """Two fixed blocks: `dist` random bytes as literals, then the same bytes again as matches of length 258 at distance `dist`
    exactly; (payload, text, bit of the second block's header)."""
    rng = random.Random(dist)
    first = bytes(rng.randrange(256) for _ in range(dist))
    w = Bits()
    w.bits(0, 1); w.bits(1, 2)
    for b in first:
        w.literal(b)
    w.length_symbol(256)
    second = w.position()
    w.bits(1, 1); w.bits(1, 2)
    code, extra = {32768: (29, 8191), 32767: (29, 8190)}[dist]  # distance code 29: 24577 + 13 extra bits
    n = 0
    while n + 258 <= dist:
        w.length_symbol(285)
        w.code(code, 5); w.bits(extra, 13)
        n += 258
    w.length_symbol(256)
    text = first + first[:n]
    return w.done(), text, second


@pytest.mark.parametrize("dist", [32768, 32767])
def test_a_second_half_that_repeats_the_first_at_the_farthest_distance(ctx, dist):
    payload, data, second = far_match_stream(dist)
    assert zlib.decompress(payload, -15) == data
    raw = wrap(payload, data)
    for starts in ([], [80 + second]):
        got, _ = inflate(ctx, raw, chunks_of(starts), len(data))
        assert got == data, (dist, starts)


# ---- member borders ---------------------------------------------------------------------------------------------------------------------
def test_member_borders_inside_and_at_the_start_of_chunks(ctx):
    raw, data, blocks, members = item("three members")
    per = [[bit for bit, _, m in blocks if m == k] for k in range(3)]
    assert all(len(p) >= 3 for p in per)
    inside = [per[0][-1], per[1][1], per[2][1]]                 # every border lies inside a chunk
    at_start = [per[0][1], per[1][0], per[1][2], per[2][0]]     # chunks that begin with a member's first block: the chunk in front read trailer and header
    for starts in (inside, at_start):
        got, info = inflate(ctx, raw, chunks_of(starts), len(data))
        assert got == data and info["members"] == 3 and info["ended"] == 1
    raw, data, blocks, members = item("an empty member in the middle")
    first = [bit for bit, _, m in blocks if m == 0]
    last = [bit for bit, _, m in blocks if m == 2]
    got, info = inflate(ctx, raw, chunks_of([first[-1], last[1]]), len(data))       # two borders in the middle chunk
    assert got == data and info["members"] == 3


def test_a_run_overflows_the_first_capacity(ctx):
    raw, data, blocks, _ = item("a run")
    assert len(data) > 8 * len(raw) + 64                        # more than 8 symbols a compressed byte
    ctx.timing(True)
    ctx.timing_reset()
    try:
        got, _ = inflate(ctx, raw, chunks_of([]), len(data))
        launches = ctx.timing_get("gzip_decode")[1]
    finally:
        ctx.timing(False)
    assert got == data
    assert launches == 2                                        # once at 8 symbols a byte, once at the format's maximum


# ---- one file in several calls ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_calls", [("fastq level 6", 2), ("fastq level 6", 3), ("three members", 3), ("sync flush points", 2)])
def test_one_file_in_several_calls(ctx, name, n_calls):
    raw, data, blocks, members = item(name)
    starts = inner_starts(blocks)
    if name == "three members":                                # the first call ends behind a trailer, the second inside a member
        edges = [0, members[0][2] * 8, [bit for bit, _, m in blocks if m == 1][-1], TO_END]
    else:
        edges = [0] + [starts[len(starts) * k // n_calls] for k in range(1, n_calls)] + [TO_END]
    stream = ctx.gzip_stream()
    got, n_members = b"", 0
    for k in range(n_calls):
        lo, hi = edges[k], edges[k + 1]
        inner = [s for s in starts if lo < s < hi]
        base = lo // 8
        piece = raw[base:] if hi == TO_END else raw[base:(hi + 7) // 8]        # comp re-based: bits count from this piece's first byte
        chunks = [(s - base * 8, e if e == TO_END else e - base * 8) for s, e in chunks_of(inner, lo, hi)]
        upto = len(data) if hi == TO_END else next(before for bit, before, _ in blocks if bit >= hi)      # (a stop behind a trailer: the next member's first block)
        part, info = inflate(ctx, piece, chunks, len(data), stream=stream)
        assert len(part) == upto - len(got)
        got += part
        n_members += info["members"]
        assert info["ended"] == (1 if k == n_calls - 1 else 0)
        assert info["end_bit"] + base * 8 == (members[-1][2] * 8 if hi == TO_END else hi)
    stream.free()
    assert got == data and n_members == len(members)


@pytest.mark.parametrize("text_at", [0, 1, 17, 4097])
def test_text_at_and_guards(ctx, text_at):
    raw, data, blocks, _ = item("fasta level 6")
    got, _ = inflate(ctx, raw, chunks_of(inner_starts(blocks)[::2]), len(data), text_at=text_at)
    assert got == data


def test_erange_names_the_room_and_leaves_the_stream(ctx):
    from metamdbg_amd import capi
    raw, data, blocks, _ = item("fastq level 1")
    starts = inner_starts(blocks)
    half = starts[len(starts) // 2]
    before = next(b for bit, b, _ in blocks if bit == half)
    stream = ctx.gzip_stream()
    first, _ = inflate(ctx, raw[:(half + 7) // 8], chunks_of([s for s in starts if s < half], 0, half), before, stream=stream)
    assert first == data[:before]
    base = half // 8
    chunks = [(s - base * 8, e if e == TO_END else e - base * 8) for s, e in chunks_of([s for s in starts if s > half], half, TO_END)]
    with pytest.raises(capi.MdbgError) as e:
        inflate(ctx, raw[base:], chunks, 0, text_at=3, room=3 + len(data) - before - 1, stream=stream)
    assert e.value.code == ERANGE and e.value.needed == len(data) - before
    rest, info = inflate(ctx, raw[base:], chunks, len(data) - before, text_at=3, stream=stream)      # the same call with room: the stream had not moved
    assert first + rest == data and info["ended"] == 1
    stream.free()


# ---- refusals: checked inputs, not faults ------------------------------------------------------------------------------------------------
def zlib_accepts(raw):
    try:
        d, out = zlib.decompressobj(31), []
        out.append(d.decompress(raw))
        while d.eof and d.unused_data[:2] == b"\x1f\x8b":
            rest = d.unused_data
            d = zlib.decompressobj(31)
            out.append(d.decompress(rest))
        return d.eof
    except zlib.error:
        return False


def refusal_cases():
    raw, data, blocks, members = item("fastq level 6")
    starts = inner_starts(blocks)
    cases = []
    moved = list(starts); moved[2] += 1
    cases.append(("a start one bit off", raw, chunks_of(moved), "chunk 2", None))
    cases.append(("a stop that is no boundary", raw, chunks_of(starts[:3], 0, starts[3] + 5), "chunk 3", "ran past the next chunk's start"))
    for p in range(starts[3] + 40, starts[3] + 4000, 37):       # a payload bit in chunk 4 that zlib refuses as well
        bad = bytearray(raw); bad[p >> 3] ^= 1 << (p & 7)
        if not zlib_accepts(bytes(bad)):
            break
    cases.append(("a flipped payload bit", bytes(bad), chunks_of(starts), "chunk", None))
    bad = bytearray(raw); bad[-8] ^= 1
    cases.append(("a wrong CRC", bytes(bad), chunks_of(starts), "chunk %d" % len(starts), "CRC-32 mismatch"))
    bad = bytearray(raw); bad[-4] ^= 1
    cases.append(("a wrong ISIZE", bytes(bad), chunks_of(starts), "chunk %d" % len(starts), "length does not match ISIZE"))
    # a second member whose first block starts with a match into the first member's text: spliced from a compressor primed with it
    a, b = data[:100000], data[60000:160000]
    c = zlib.compressobj(6, zlib.DEFLATED, -15, zdict=a[-32768:])
    spliced = member(a) + wrap(c.compress(b) + c.flush(), b)
    sb, sm = file_blocks_of_first_member(member(a))
    second = (sm + 10) * 8
    cases.append(("a back-reference across a member border", spliced, chunks_of([sb[1]]), "chunk 1", "reference before the member's start"))
    cases.append(("the same with the border at a chunk's start", spliced, chunks_of([sb[1], second]), "chunk 2", "reference before the member's start"))
    return raw, data, starts, cases


def file_blocks_of_first_member(raw):
    blocks, members = file_blocks(raw)
    return [bit for bit, _, _ in blocks], members[0][2]


def test_refusals_and_the_call_after_them(ctx):
    from metamdbg_amd import capi
    raw, data, starts, cases = refusal_cases()
    for name, bad, chunks, where, why in cases:
        if name not in ("a start one bit off", "a stop that is no boundary"):
            assert not zlib_accepts(bad), name                  # the very bytes sent to the device are bad by zlib's account too
        with pytest.raises(capi.MdbgError) as e:
            inflate(ctx, bad, chunks, len(data) + 200000)
        assert e.value.code == EINVAL, name
        assert where in str(e.value) and "does not decode" in str(e.value), (name, str(e.value))
        if why:
            assert why in str(e.value), (name, str(e.value))
        assert inflate(ctx, raw, chunks_of(starts), len(data))[0] == data, name      # a fresh stream of the same context works


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
    lens = [LENGTHS[i % len(LENGTHS)] if i % 40 else 3000 for i in range(600)]
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
    assert n == 600
    want = describe(ctx, r, n)
    want["fastx_info"] = r.fastx_info
    r.free(); plain.free()
    raw = member(text, 6)
    blocks, _ = file_blocks(raw)
    comp = ctx.bytes_from_host(raw)
    buf = ctx.bytes_create(len(text))
    stream = ctx.gzip_stream()
    assert ctx.inflate_gzip(stream, comp, chunks_of(inner_starts(blocks)), buf)["n_text"] == len(text)
    r = ctx.reads_from_fastx_bytes(buf)                        # no synchronisation in between
    got = describe(ctx, r, n)
    got["fastx_info"] = r.fastx_info
    r.free(); buf.free(); comp.free(); stream.free()
    for k in want:
        assert same(got[k], want[k]), k


def test_bytes_copy_checks_its_ranges(ctx):
    from metamdbg_amd import capi
    a = ctx.bytes_from_host(b"0123456789")
    b = ctx.bytes_from_host(b"abcdefghij")
    ctx.bytes_copy(b, 2, a, 5, 4)
    ctx.bytes_copy(b, 10, a, 0, 0)
    ctx.bytes_copy(a, 0, a, 6, 4)                              # one buffer, apart
    assert b.download(0, 10) == b"ab5678ghij" and a.download(0, 10) == b"6789456789"
    for dst, dst_at, src, src_at, n in ((b, 7, a, 0, 4), (b, 0, a, 7, 4), (b, 11, a, 0, 0), (b, 0, a, 11, 0), (a, 0, a, 3, 4), (a, 2, a, 2, 1)):
        with pytest.raises(capi.MdbgError) as e:
            ctx.bytes_copy(dst, dst_at, src, src_at, n)
        assert e.value.code == EINVAL
    assert b.download(0, 10) == b"ab5678ghij"
    a.free(); b.free()
