"""mdbg_spans_stitch / mdbg_reads_stitch_ranges / mdbg_sequences_to_fasta_bytes (csrc/stitch.hip, csrc/stitch_dev.hpp): contig sequences put
together from oriented pieces of the packed reads on the device, and the FASTA text of them.  Expected values: the text the reference wrote
for tests/golden/contig_stitch (ToBasespaceGfa::CreateBaseContigsFunctor over DnaBitset2 pieces, written by the generator committed there)
and the numpy restatement tests/stitch_model.py, which tests/test_contig_stitch_model.py compares with the same text on the CPU.
Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from metamdbg_amd import capi, synth
from tests import extract_model as EM
from tests import stitch_model as SM

pytestmark = pytest.mark.gpu

FORMS = ((capi.SEQ_BITSET, "bitset"), (capi.SEQ_ASCII, "ascii"))


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def rand_seq(rng, n: int) -> bytes:
    return bytes(synth.CODE2ASCII[rng.integers(0, 4, int(n))])


def scan(ctx, reads, l, density, hpc, no_end_trim=False):
    return ctx.scan(reads, K=l, density=density, hpc=hpc, apply_read_filters=False, no_end_trim=no_end_trim)


def host(sq, n: int, form: int) -> dict:
    got = sq.to_host()
    assert sq.info() == dict(n=n, n_bases=int(got["lengths"].sum()), n_bytes=len(got["bytes"]), form=form)
    return got


def stitch_ranges(ctx, reads, rg, off, form: int) -> dict:
    rg = np.asarray(rg, dtype=np.int64).reshape(-1, 4)
    sq = ctx.reads_stitch_ranges(reads, rg[:, 0], rg[:, 1], rg[:, 2], rg[:, 3], off, form)
    got = host(sq, len(off) - 1, form)
    sq.close()
    return got


def check_ranges(ctx, reads, seqs, contigs, what: str) -> dict:
    """contigs: per contig a list of (read, start, length, reversed); both forms against the model; returns the ASCII result."""
    rg = np.array([p for c in contigs for p in c], dtype=np.int64).reshape(-1, 4)
    off = np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.uint64)
    strings = SM.range_contig_strings(seqs, rg, off)
    for form, name in FORMS:
        got = stitch_ranges(ctx, reads, rg, off, form)
        EM.assert_equal(got, SM.layout(strings, form), f"{what}, {name}")
    return got


def texts(got: dict, form: int = capi.SEQ_ASCII) -> list[bytes]:
    """Every sequence's meaningful bytes: its characters, or its DnaBitset2 bytes."""
    off, n = got["byte_offsets"].astype(np.int64), got["lengths"].astype(np.int64)
    if form == capi.SEQ_BITSET:
        n = (n + 3) // 4
    return [got["bytes"][o:o + k].tobytes() for o, k in zip(off[:-1], n)]


# ---- 1. the reference's text, the whole chain ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ("fresh_scan", "concat"))
@pytest.mark.parametrize("cfg", SM.MANIFEST["configs"], ids=[c["name"] for c in SM.MANIFEST["configs"]])
def test_fixture_whole_chain(ctx, cfg, source):
    """reads -> mdbg_scan -> mdbg_kminmer_spans -> mdbg_spans_stitch (BITSET) -> mdbg_sequences_to_fasta_bytes -> mdbg_bytes_download against
    the text CreateBaseContigsFunctor wrote, byte for byte; the ASCII form and both forms' arrays against the model."""
    seqs, want_spans, contigs, want = SM.load(cfg)
    reads = ctx.reads_from_ascii(seqs)
    hpc, trim0 = bool(cfg["hpc"]), cfg["trim"] == 0
    if source == "fresh_scan":
        mins = scan(ctx, reads, cfg["l"], cfg["density"], hpc, trim0)
    else:
        half = len(seqs) // 2
        mins = ctx.minimizers_concat([scan(ctx, ctx.reads_from_ascii(part), cfg["l"], cfg["density"], hpc, trim0) for part in (seqs[:half], seqs[half:])])
    sp = ctx.kminmer_spans(reads, mins, K=cfg["l"], hpc=hpc, k=cfg["k"])
    spans = sp.to_host()
    for f in ("window_offsets", "reversed", "pos_start", "pos_end", "seq_length_start", "seq_length_end"):
        assert np.array_equal(spans[f], want_spans[f]), f                # the windows the fixture's contigs count are the library's
    pieces, offsets = capi.stitch_pieces([[((r, w) if p else None, v) for r, w, v, p in c] for c in contigs], spans["window_offsets"])
    assert len(offsets) - 1 == cfg["n_contigs"] and len(pieces) == cfg["n_positions"]
    for form, name in FORMS:
        sq = ctx.spans_stitch(reads, sp, pieces, offsets, form)
        got = host(sq, cfg["n_contigs"], form)
        EM.assert_equal(got, SM.layout(SM.contig_strings(seqs, spans, pieces, offsets, form), form), f"{cfg['name']} {name}")
        EM.unpadded(got, form)
        if form == capi.SEQ_BITSET:
            text = ctx.sequences_to_fasta_bytes(sq, want["names"], want["flags"])
            assert text.n == cfg["n_text_bytes"]
            got_text = text.download(0, text.n)
            if got_text != want["text"].tobytes():
                at = int(np.flatnonzero(np.frombuffer(got_text, np.uint8) != want["text"])[0])
                raise AssertionError(f"the text differs first at byte {at} of {text.n}: {got_text[max(0, at - 20):at + 20]!r} against {want['text'].tobytes()[max(0, at - 20):at + 20]!r}")
            # names and flags left out: 0, 1, 2 ... and "l"
            plain = ctx.sequences_to_fasta_bytes(sq)
            assert plain.download(0, plain.n) == SM.fasta_text(SM.contig_strings(seqs, spans, pieces, offsets, EM.BITSET))
        sq.close()


# ---- 2. stitch against extract -------------------------------------------------------------------------------------------------------------
def test_stitch_equals_the_concatenation_of_what_extract_returns(ctx):
    """The stitch of a contig = the model's concatenation (flip, invalid rule) of what mdbg_spans_extract returns for its pieces; the same
    batch again with the contigs in permuted order."""
    rng = np.random.default_rng(131)
    seqs = [rand_seq(rng, int(n)) for n in rng.integers(200, 4000, 25)] + [rand_seq(rng, 400) + b"NN" + rand_seq(rng, 300) + b"K" + rand_seq(rng, 500)]
    reads = ctx.reads_from_ascii(seqs)
    sp = ctx.kminmer_spans(reads, scan(ctx, reads, 13, 0.1, True), K=13, hpc=True, k=4)
    n_win = sp.info()["n_windows"]
    assert n_win > 1000
    contigs = [[(None if rng.random() < 0.1 else int(w), int(rng.integers(0, 2))) for w in rng.integers(0, n_win, int(rng.integers(0, 30)))] for _ in range(300)]
    last = int(sp.to_host()["window_offsets"][-2])
    contigs += [[(w, w & 1) for w in range(last, n_win)], [(w, 1 - (w & 1)) for w in range(n_win - 1, last - 1, -1)]]       # every window of the read with N and K
    first = {}
    for order in (np.arange(len(contigs)), rng.permutation(len(contigs))):
        pieces, offsets = capi.stitch_pieces([contigs[i] for i in order])
        real = pieces["window"] != capi.STITCH_NONE
        ex = texts(ctx.spans_extract(reads, sp, pieces["window"][real], pieces["part"][real], capi.SEQ_ASCII).to_host())
        for form, name in FORMS:
            by_piece = iter(ex)
            strings = []
            for c in range(len(order)):
                s = b""
                for p in pieces[int(offsets[c]):int(offsets[c + 1])]:
                    if p["window"] == capi.STITCH_NONE:
                        continue
                    t = next(by_piece)
                    if form == capi.SEQ_BITSET:
                        t = t.replace(b"N", b"A")
                    s += SM.revcomp(t) if p["flip"] else t
                strings.append(s)
            got = host(ctx.spans_stitch(reads, sp, pieces, offsets, form), len(order), form)
            EM.assert_equal(got, SM.layout(strings, form), f"against extract, {name}")
            if form in first:
                assert texts(got, form) == [first[form][i] for i in order]
            else:
                first[form] = texts(got, form)
    assert any(b"N" in t for t in first[capi.SEQ_ASCII])


# ---- 3. the ranges entry -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch(ctx):
    rng = np.random.default_rng(141)
    body = lambda n: rand_seq(rng, n)
    seqs = [body(70_040), body(5000), body(333), body(40) + b"N" * 50 + body(200) + b"NNN" + body(100), body(150) + b"N", b"N" + body(150), body(64), body(1)]
    return seqs, ctx.reads_from_ascii(seqs)


def cut(read: int, length: int, size: int) -> list:
    return [(read, at, min(size, length - at), 0) for at in range(0, length, size)]


def test_a_read_whole_and_cut_into_pieces_and_put_back_together(ctx, batch):
    seqs, reads = batch
    for r in (1, 3):
        L = len(seqs[r])
        contigs = [[(r, 0, L, 0)], [(r, 0, L, 1)]]
        for size in (1, 7, 31, 32, 33):
            contigs.append(cut(r, L, size))                                              # equals the read
            contigs.append([(a, b, c, 1) for a, b, c, _ in reversed(cut(r, L, size))])  # reversed, the order reversed: its reverse complement
        got = texts(check_ranges(ctx, reads, seqs, contigs, f"read {r} in pieces"))
        whole = seqs[r].translate(EM.KNOWN)
        assert got[0] == whole and got[1] == SM.revcomp(whole)
        assert all(t == whole for t in got[2::2]) and all(t == SM.revcomp(whole) for t in got[3::2])


def test_one_base_pieces_empty_pieces_and_contigs_without_pieces(ctx, batch):
    seqs, reads = batch
    rng = np.random.default_rng(143)
    forty = [(3, int(s), 1, int(v)) for s, v in zip(rng.integers(30, 110, 40), rng.integers(0, 2, 40))]           # a word of 32 pieces, N among them
    empty = (2, 5, 0, 0)
    contigs = [forty, [], [empty, (2, 0, 50, 0), empty, empty, (1, 4900, 100, 1), empty], [], [empty, empty], [(7, 0, 1, 1)], [], [(6, 0, 64, 0), (6, 64, 0, 1)], []]
    got = check_ranges(ctx, reads, seqs, contigs, "one-base and empty pieces")
    assert list(got["lengths"]) == [40, 0, 150, 0, 0, 1, 0, 64, 0]
    assert list(np.diff(got["byte_offsets"].astype(np.int64))) == [40, 0, 152, 0, 0, 8, 0, 64, 0]
    check_ranges(ctx, reads, seqs, [[], []], "nothing but contigs without pieces")
    for n in (1, 31, 32, 33, 63, 64, 65, 4097):                                           # contigs of these bases out of pieces of at most 9
        contig = []
        while sum(p[2] for p in contig) < n:
            k = min(int(rng.integers(0, 10)), n - sum(p[2] for p in contig))
            contig.append((1, int(rng.integers(0, 5000 - k)), k, int(rng.integers(0, 2))))
        check_ranges(ctx, reads, seqs, [contig, [(2, 0, 9, 0)]], f"{n} bases")


def test_one_long_contig_beside_many_short(ctx, batch):
    """A 70 kb read as one contig of 700 pieces beside 5 000 contigs of one 50-base piece: the output words are dealt to the waves."""
    seqs, reads = batch
    rng = np.random.default_rng(145)
    short = [[(int(r), int(rng.integers(0, len(seqs[r]) - 50)), 50, int(v))] for r, v in zip(rng.integers(0, 3, 5000), rng.integers(0, 2, 5000))]
    for v in (0, 1):
        long = cut(0, 70_000, 100)
        if v:
            long = [(a, b, c, 1) for a, b, c, _ in reversed(long)]
        got = texts(check_ranges(ctx, reads, seqs, short[:2500] + [long] + short[2500:] + [[(0, 0, 70_040, v)]], f"skewed, reversed {v}"))
        assert got[2500] == (SM.revcomp(seqs[0][:70_000]) if v else seqs[0][:70_000])


def test_reads_with_n_islands(ctx, batch):
    """Ranges that start or end on, just before and just behind a masked base: N in the characters, code 0 in the bitset, both orientations."""
    seqs, reads = batch
    contigs = []
    for r in (3, 4, 5):
        s = seqs[r]
        bad = np.flatnonzero(np.frombuffer(s, np.uint8) & 8)
        edges = sorted({0, len(s)} | {int(x) for b in bad for x in (b - 1, b, b + 1) if 0 <= x <= len(s)})
        for i, a in enumerate(edges):
            contigs.append([(r, a, b - a, (i + j) & 1) for j, b in enumerate(edges) if a <= b and (b - a) % 5 in (0, 1, 3)])
    assert 50 < len(contigs) < 500
    got = check_ranges(ctx, reads, seqs, contigs, "islands")
    assert any(b"N" in t for t in texts(got))
    # ... and in the text: DnaBitset2::to_string knows no N
    sq = ctx.reads_stitch_ranges(reads, [3, 3], [35, 35], [60, 60], [0, 1], [0, 1, 2])
    text = ctx.sequences_to_fasta_bytes(sq, [5, 6], [1, 0])
    body = seqs[3][35:95].translate(EM.KNOWN).replace(b"N", b"A")
    assert text.download(0, text.n) == b">ctg5c\n" + body + b"\n>ctg6l\n" + SM.revcomp(seqs[3][35:95].translate(EM.KNOWN)).replace(b"N", b"A") + b"\n"


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """Each is MDBG_EINVAL with a message that names piece and contig, *out stays untouched, and a correct call straight afterwards succeeds."""
    L = capi.lib()
    rng = np.random.default_rng(151)
    seqs = [rand_seq(rng, int(n)) for n in rng.integers(300, 3000, 20)]
    other = [rand_seq(rng, len(s) + 1 + i % 3) for i, s in enumerate(seqs)]           # as many reads, other lengths
    reads, reads_other = ctx.reads_from_ascii(seqs), ctx.reads_from_ascii(other)
    sp = ctx.kminmer_spans(reads, scan(ctx, reads, 13, 0.1, True), K=13, hpc=True, k=4)
    sp_other = ctx.kminmer_spans(reads_other, scan(ctx, reads_other, 13, 0.1, True), K=13, hpc=True, k=4)
    spans = sp.to_host()
    n_win = sp.info()["n_windows"]
    good, good_off = capi.stitch_pieces([[(int(w), int(w) & 1) for w in range(c, min(c + 5, n_win))] for c in range(0, 60, 5)])
    want = SM.layout(SM.contig_strings(seqs, spans, good, good_off, EM.BITSET), EM.BITSET)
    SENTINEL = 0x5A5A5A5A
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def outcome(rc, out_h, piece=None, contig=None, says=None):
        assert rc == -1, rc                                                           # MDBG_EINVAL
        assert out_h.value == SENTINEL
        msg = (L.mdbg_last_error(ctx.h) or b"").decode()
        if piece is not None:
            assert f"piece {piece} " in msg and f"contig {contig}" in msg, msg
        if says:
            assert says in msg, msg
        EM.assert_equal(ctx.spans_stitch(reads, sp, good, good_off).to_host(), want, "a correct call behind a refusal")

    def refused_piece(at, window, part, flip=0, form=capi.SEQ_BITSET, reads_h=None, spans_h=None, named=True):
        pc = good.copy()
        pc[at] = (window, part, flip)
        out_h = C.c_void_p(SENTINEL)
        rc = L.mdbg_spans_stitch(ctx.h, reads_h or reads.h, spans_h or sp.h, ptr(pc), ptr(good_off), len(good_off) - 1, form, C.byref(out_h))
        outcome(rc, out_h, at if named else None, at // 5)

    def refused_range(at, rd, start, length):
        rg = np.zeros(40, capi.SEQ_RANGE)
        rg["length"] = 10
        rg[at] = (rd, start, length, 0)
        off = np.arange(0, 41, 4, dtype=np.uint64)
        out_h = C.c_void_p(SENTINEL)
        outcome(L.mdbg_reads_stitch_ranges(ctx.h, reads.h, ptr(rg), ptr(off), len(off) - 1, 0, C.byref(out_h)), out_h, at, at // 4)

    def refused_offsets(off, says):
        off = np.array(off, dtype=np.uint64)
        out_h = C.c_void_p(SENTINEL)
        outcome(L.mdbg_spans_stitch(ctx.h, reads.h, sp.h, ptr(good), ptr(off), len(off) - 1, 0, C.byref(out_h)), out_h, says=says)

    refused_piece(7, 3, 3)                                           # a bad part
    refused_piece(12, n_win, 0)                                      # a window index equal to n_windows
    refused_piece(len(good) - 1, 2 ** 63, 1, 1)                      # ... far beyond, in the last piece
    refused_piece(0, 0, 0, spans_h=sp_other.h)                       # spans of another read set: as many reads, other lengths
    refused_piece(0, 0, 0, reads_h=ctx.reads_from_ascii(seqs[:-1]).h, named=False)      # ... another number of reads
    refused_piece(0, 0, 0, form=2, named=False)                      # form out of range
    refused_range(11, 2, len(seqs[2]) - 9, 10)                       # a range behind its read's end
    refused_range(0, 2, 0xFFFFFFFF, 2)                               # start + length wraps 32 bits
    refused_range(39, len(seqs), 0, 0)                               # a read index equal to n_reads, although the piece is empty
    refused_offsets([0, 5, 4, 60], "decrease")                       # piece_offsets decreasing
    refused_offsets([1, 5, 60], "piece_offsets[0]")                  # ... not starting at 0
    # two offending pieces: the first is named
    pc = good.copy()
    pc[40] = (0, 7, 0)
    pc[9] = (n_win + 5, 0, 0)
    out_h = C.c_void_p(SENTINEL)
    outcome(L.mdbg_spans_stitch(ctx.h, reads.h, sp.h, ptr(pc), ptr(good_off), len(good_off) - 1, 0, C.byref(out_h)), out_h, 9, 1)
    # MDBG_STITCH_NONE: the other fields are not looked at
    pc = good.copy()
    pc[3] = (capi.STITCH_NONE, 77, 5)
    assert list(ctx.spans_stitch(reads, sp, pc, good_off).to_host()["lengths"][1:]) == list(want["lengths"][1:])
    # the text: ASCII-form input, a flag of 3, null arguments
    sq_ascii, sq = ctx.spans_stitch(reads, sp, good, good_off, capi.SEQ_ASCII), ctx.spans_stitch(reads, sp, good, good_off)
    flags = np.zeros(len(good_off) - 1, np.uint8)
    out_h, n = C.c_void_p(SENTINEL), C.c_uint64(77)
    assert L.mdbg_sequences_to_fasta_bytes(ctx.h, sq_ascii.h, None, None, C.byref(out_h), C.byref(n)) == -1 and out_h.value == SENTINEL and n.value == 77
    assert "MDBG_SEQ_BITSET" in L.mdbg_last_error(ctx.h).decode()
    flags[4] = 3
    assert L.mdbg_sequences_to_fasta_bytes(ctx.h, sq.h, None, ptr(flags), C.byref(out_h), C.byref(n)) == -1 and out_h.value == SENTINEL
    assert "sequence 4" in L.mdbg_last_error(ctx.h).decode()
    assert L.mdbg_sequences_to_fasta_bytes(ctx.h, None, None, None, C.byref(out_h), None) == -1 and L.mdbg_sequences_to_fasta_bytes(ctx.h, sq.h, None, None, None, None) == -1
    assert L.mdbg_spans_stitch(ctx.h, None, sp.h, ptr(good), ptr(good_off), 1, 0, C.byref(out_h)) == -1 and out_h.value == SENTINEL
    assert L.mdbg_spans_stitch(ctx.h, reads.h, sp.h, None, ptr(good_off), 1, 0, C.byref(out_h)) == -1 and out_h.value == SENTINEL
    assert L.mdbg_spans_stitch(ctx.h, reads.h, sp.h, ptr(good), None, 1, 0, C.byref(out_h)) == -1 and out_h.value == SENTINEL
    assert L.mdbg_reads_stitch_ranges(ctx.h, reads.h, None, ptr(good_off), 1, 0, C.byref(out_h)) == -1 and out_h.value == SENTINEL
    assert L.mdbg_spans_stitch(ctx.h, reads.h, sp.h, ptr(good), ptr(good_off), 1, 0, None) == -1
    flags[4] = 2
    text = ctx.sequences_to_fasta_bytes(sq, None, flags)
    assert text.download(0, text.n) == SM.fasta_text(SM.contig_strings(seqs, spans, good, good_off, EM.BITSET), None, flags)


# ---- 5. contexts, zero contigs, timers, attributes -------------------------------------------------------------------------------------------
def test_two_contexts_alternating(ctx):
    rng = np.random.default_rng(161)
    other = capi.Context(0)
    try:
        sides = []
        for c in (ctx, other):
            seqs = [rand_seq(rng, int(n)) for n in rng.integers(100, 4000, 40)]
            contigs = []
            for _ in range(200):
                rd = rng.integers(0, len(seqs), int(rng.integers(0, 8)))
                ln = [int(rng.integers(0, min(len(seqs[r]), 333) + 1)) for r in rd]
                contigs.append([(int(r), int(rng.integers(0, len(seqs[r]) - l + 1)), l, int(rng.integers(0, 2))) for r, l in zip(rd, ln)])
            sides.append((c, seqs, c.reads_from_ascii(seqs), contigs))
        for turn in range(3):
            for c, seqs, reads, contigs in sides:
                check_ranges(c, reads, seqs, contigs[turn * 30:], f"turn {turn}")
                rg = np.array([p for k in contigs[:50] for p in k])
                off = np.concatenate([[0], np.cumsum([len(k) for k in contigs[:50]])])
                names, flags = np.arange(50) * 1000003 % 2 ** 32, np.arange(50) % 3
                text = c.sequences_to_fasta_bytes(c.reads_stitch_ranges(reads, *rg.T, off), names, flags)
                assert text.download(0, text.n) == SM.fasta_text(SM.range_contig_strings(seqs, rg, off), names, flags)
    finally:
        other.close()


def test_zero_contigs_timers_and_kernel_attributes(ctx, batch):
    seqs, reads = batch
    for form, _ in FORMS:
        got = stitch_ranges(ctx, reads, np.zeros((0, 4)), np.zeros(1, np.uint64), form)
        assert list(got["byte_offsets"]) == [0] and len(got["bytes"]) == 0 and len(got["lengths"]) == 0
    sq = ctx.reads_stitch_ranges(reads, [], [], [], [], [0])
    text = ctx.sequences_to_fasta_bytes(sq)
    assert text.n == 0 and text.download(0, 0) == b""
    ctx.timing(True)
    ctx.timing_reset()
    try:
        sq = ctx.reads_stitch_ranges(reads, [0, 0, 2], [5, 7, 0], [1000, 1000, 31], [0, 1, 0], [0, 2, 3])
        text = ctx.sequences_to_fasta_bytes(sq)
        ctx.synchronize()
        for name in ("stitch_plan", "stitch_copy", "fasta_plan", "fasta_write"):
            assert ctx.timing_get(name)[1] == 1, name
    finally:
        ctx.timing(False)
    assert list(sq.to_host()["byte_offsets"]) == [0, 504, 512] and text.n == 7 + 2001 + 7 + 32
    p = sq.device_ptrs()
    assert all(p.values()) and p["bytes"] % 16 == 0
    for name in ("stitch_plan", "stitch_plan_ranges", "stitch_contigs", "stitch_copy", "fasta_plan", "fasta_write"):
        a = ctx.kernel_attributes(name)
        assert a["scratch"] == 0 and a["static_lds"] == 0 and a["role"] == 2, (name, a)
