"""mdbg_spans_extract / mdbg_reads_extract_ranges (csrc/extract.hip, csrc/extract_dev.hpp): the oriented sequences of (window, part)
requests, or of ranges given by the caller, cut out of the packed reads on the device and laid out as DnaBitset2 keeps them or as
characters.  Expected values: the reference's own answers under tests/golden/kminmer_sequences (ToBasespaceGfa::extractKminmerSequence +
DnaBitset2, written by the generator committed there) and the numpy restatement tests/extract_model.py, which
tests/test_kminmer_sequences_model.py compares with the same answers on the CPU.
Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import pytest

from metamdbg_amd import capi, synth
from tests import extract_model as EM
from tests import helpers as H

pytestmark = pytest.mark.gpu

FIX = os.path.join(H.GOLDEN, "kminmer_sequences")
with open(os.path.join(FIX, "manifest.json")) as _f:
    MANIFEST = json.load(_f)
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


def pieces(got: dict) -> list[bytes]:
    """Every sequence's bytes, padding included."""
    off = got["byte_offsets"].astype(np.int64)
    return [got["bytes"][off[i]:off[i + 1]].tobytes() for i in range(len(off) - 1)]


def extract_ranges(ctx, reads, rg: np.ndarray, form: int) -> dict:
    sq = ctx.reads_extract_ranges(reads, rg[:, 0], rg[:, 1], rg[:, 2], rg[:, 3], form)
    got = sq.to_host()
    assert sq.info() == dict(n=len(rg), n_bases=int(rg[:, 2].sum()), n_bytes=len(got["bytes"]), form=form)
    sq.close()
    return got


def check_ranges(ctx, reads, seqs, rg, what: str) -> None:
    rg = np.asarray(rg, dtype=np.int64).reshape(-1, 4)
    for form, name in FORMS:
        EM.assert_equal(extract_ranges(ctx, reads, rg, form), EM.expected(seqs, rg[:, 0], rg[:, 1], rg[:, 2], rg[:, 3], form), f"{what}, {name}")


# ---- 1. the reference's answers ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_reads():
    with open(os.path.join(FIX, MANIFEST["reads"]), "rb") as f:
        reads = f.read().split(b"\n")[:-1]
    assert len(reads) == MANIFEST["n_reads"]
    return reads


@pytest.mark.parametrize("source", ("fresh_scan", "concat"))
@pytest.mark.parametrize("cfg", MANIFEST["configs"], ids=[c["name"] for c in MANIFEST["configs"]])
def test_fixture_from_the_reference(ctx, fixture_reads, cfg, source):
    """reads -> mdbg_scan -> mdbg_kminmer_spans -> mdbg_spans_extract against getKminmers + extractKminmerSequence + DnaBitset2, byte for byte,
    the requests as the fixture lists them; from a fresh scan output and from the mdbg_minimizers_concat of the scans of the two halves of the
    reads; then permuted, and with every request twice."""
    want = np.load(os.path.join(FIX, cfg["name"] + ".npz"))
    seqs = [fixture_reads[i] for i in cfg["reads"]]
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
        assert np.array_equal(spans[f], want[f]), f                     # the windows the fixture's requests count are the library's
    windows, parts = want["req_window"], want["req_part"]
    assert len(windows) == cfg["n_requests"]
    first = {}
    for form, name in FORMS:
        sq = ctx.spans_extract(reads, sp, windows, parts, form)
        got = sq.to_host()
        assert sq.info() == dict(n=cfg["n_requests"], n_bases=cfg["n_bases"], n_bytes=len(got["bytes"]), form=form)
        assert np.array_equal(got["lengths"], want["lengths"])
        if form == capi.SEQ_BITSET:
            assert np.array_equal(EM.unpadded(got, EM.BITSET), want["bitset"]), "DnaBitset2's bytes"
        EM.assert_equal(got, EM.expected_requests(seqs, spans, windows, parts, form), f"{cfg['name']} {name}")
        first[form] = pieces(got)
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(windows))
    twice = np.repeat(np.arange(len(windows)), 2)
    for form, name in FORMS:
        for order in (perm, twice):
            got = ctx.spans_extract(reads, sp, windows[order], parts[order], form).to_host()
            assert np.array_equal(got["lengths"], want["lengths"][order]) and pieces(got) == [first[form][i] for i in order], name
            EM.unpadded(got, form)                                      # offsets at multiples of 8, padding zero


# ---- 2. ranges -----------------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 70_000)
STARTS = (0, 1, 31, 32, 33)


@pytest.fixture(scope="module")
def plain_batch(ctx):
    """Reads of A, C, G, T only: the batch carries no invalid mask (the kernel's null-mask branch)."""
    rng = np.random.default_rng(51)
    seqs = [rand_seq(rng, 70_040), rand_seq(rng, 300_001)] + [rand_seq(rng, n) for n in (1, 31, 32, 33, 63, 64, 65, 100, 2047, 2048, 2049, 5000)]
    return seqs, ctx.reads_from_ascii(seqs)


def test_ranges_lengths_starts_and_orientations(ctx, plain_batch):
    seqs, reads = plain_batch
    rg = [(0, s, n, v) for n in LENGTHS for s in STARTS for v in (0, 1)]
    assert len(rg) == 150
    check_ranges(ctx, reads, seqs, rg, "lengths x starts")


def test_ranges_at_a_reads_last_base_and_whole_reads(ctx, plain_batch):
    seqs, reads = plain_batch
    at_end = [(r, len(s) - n, n, v) for r, s in enumerate(seqs) for n in LENGTHS if n <= len(s) for v in (0, 1)]
    whole = [(r, 0, len(s), v) for r, s in enumerate(seqs) for v in (0, 1)]          # v = 0: LoadUnitigsFunctor's DnaBitset2(read._seq)
    check_ranges(ctx, reads, seqs, at_end + whole, "at the end and whole")
    # the last read of the batch: nothing follows its words
    last = len(seqs) - 1
    check_ranges(ctx, reads, seqs, [(last, len(seqs[last]) - n, n, v) for n in (1, 31, 33, 64, 5000) for v in (0, 1)], "the batch's last read")


@pytest.mark.parametrize("n", (0, 1, 64, 65))
def test_number_of_requests(ctx, plain_batch, n):
    seqs, reads = plain_batch
    rng = np.random.default_rng(53 + n)
    rd = rng.integers(2, len(seqs), n)
    ln = np.array([rng.integers(0, len(seqs[r]) + 1) for r in rd], dtype=np.int64)
    st = np.array([rng.integers(0, len(seqs[r]) - l + 1) for r, l in zip(rd, ln)], dtype=np.int64)
    rg = np.stack([rd, st, ln, rng.integers(0, 2, n)], axis=1).reshape(-1, 4)
    check_ranges(ctx, reads, seqs, rg, f"n = {n}")
    if n == 0:
        got = extract_ranges(ctx, reads, rg, capi.SEQ_BITSET)
        assert list(got["byte_offsets"]) == [0] and len(got["bytes"]) == 0 and len(got["lengths"]) == 0


def test_one_long_range_among_many_short(ctx, plain_batch):
    """One range of 300 kb among 5000 of 40 bases: the output words are dealt to the waves, not the requests."""
    seqs, reads = plain_batch
    rng = np.random.default_rng(55)
    rd = rng.integers(0, len(seqs), 5000)
    rd[[len(s) < 40 for s in (seqs[r] for r in rd)]] = 0
    st = np.array([rng.integers(0, len(seqs[r]) - 40 + 1) for r in rd], dtype=np.int64)
    rg = np.stack([rd, st, np.full(5000, 40), rng.integers(0, 2, 5000)], axis=1)
    for v in (0, 1):
        both = np.concatenate([rg[:2500], [[1, 1, 300_000, v]], rg[2500:]])
        check_ranges(ctx, reads, seqs, both, f"skewed, reversed {v}")


# ---- 3. masks ------------------------------------------------------------------------------------------------------------------------
def test_invalid_mask_case_and_iupac(ctx):
    """N runs (code 0 and 'N' in both orientations), "aA" and IUPAC letters: a lower-case letter or R / S / W comes out as the base its 2-bit
    code names (the header's deliberate difference), K / M / Y / n (bit 3) as N."""
    rng = np.random.default_rng(57)
    body = lambda n: rand_seq(rng, n)
    seqs = [body(300), body(40) + b"N" * 50 + body(200) + b"NNN" + body(100), body(31) + b"aA" * 20 + body(120) + b"AaAAaa" + body(64),
            body(100) + b"CSCSSc" + body(90) + b"GRrRK" + body(77) + b"TtYyWw" + body(50), body(50) + b"GNG" + body(61) + b"NGGN" + body(200) + b"gNnG" + body(30),
            body(2040) + b"GGGGNNNNNNGGGG" + body(300), b"N" + body(150), body(150) + b"N", b"N" * 70, body(500)]
    reads = ctx.reads_from_ascii(seqs)
    rg = []
    for r, s in enumerate(seqs):
        bad = np.flatnonzero(np.frombuffer(s, np.uint8) & 8)
        edges = sorted({0, len(s)} | {int(x) for b in bad[:40] for x in (b - 1, b, b + 1) if 0 <= x <= len(s)})
        for a in edges:                         # ranges that start or end on, just before and just behind a masked base
            for b in edges:
                if a <= b and (b - a) % 7 in (0, 1, 3):
                    rg += [(r, a, b - a, 0), (r, a, b - a, 1)]
        rg += [(r, 0, len(s), 0), (r, 0, len(s), 1)]
    assert 500 < len(rg) < 20_000
    check_ranges(ctx, reads, seqs, rg, "masks")
    got = extract_ranges(ctx, reads, np.array([(8, 3, 50, 1), (3, 100, 6, 0), (3, 196, 5, 1)]), capi.SEQ_ASCII)
    assert pieces(got)[0].rstrip(b"\0") == b"N" * 50 and pieces(got)[1] == b"CCCCCC\0\0" and pieces(got)[2] == b"NGGGC\0\0\0"      # CSCSSc; GRrRK reverse-complemented


# ---- 4. (window, part) requests on seeded reads ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hpc", (False, True), ids=("plain", "hpc"))
@pytest.mark.parametrize("k", (2, 4, 13))
def test_every_window_and_part(ctx, k, hpc):
    rng = np.random.default_rng(61 + k)
    seqs = [rand_seq(rng, int(n)) for n in rng.integers(100, 3000, 30)] + [rand_seq(rng, 500) + b"NN" + rand_seq(rng, 700), rand_seq(rng, 20)]
    reads = ctx.reads_from_ascii(seqs)
    sp = ctx.kminmer_spans(reads, scan(ctx, reads, 13, 0.1, hpc), K=13, hpc=hpc, k=k)
    spans = sp.to_host()
    n_win = len(spans["reversed"])
    assert n_win > 1000 and 0 < spans["reversed"].sum() < n_win
    windows, parts = np.tile(np.arange(n_win), 3), np.repeat([capi.SEQ_ENTIRE, capi.SEQ_LEFT, capi.SEQ_RIGHT], n_win)
    for form, name in FORMS:
        got = ctx.spans_extract(reads, sp, windows, parts, form).to_host()
        EM.assert_equal(got, EM.expected_requests(seqs, spans, windows, parts, form), f"k {k} hpc {hpc} {name}")
    # an ENTIRE sequence begins with its LEFT and ends with its RIGHT part
    text = pieces(ctx.spans_extract(reads, sp, windows, parts, capi.SEQ_ASCII).to_host())
    for w in range(0, n_win, 37):
        e, l, r = (text[w + p * n_win].rstrip(b"\0") for p in range(3))
        assert e.startswith(l) and e.endswith(r) and len(l) == spans["seq_length_start"][w] and len(r) == spans["seq_length_end"][w]


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """Each is MDBG_EINVAL with a message that names the request, *out stays untouched, and a correct call straight afterwards succeeds."""
    L = capi.lib()
    rng = np.random.default_rng(71)
    seqs = [rand_seq(rng, int(n)) for n in rng.integers(300, 3000, 20)]
    other = [rand_seq(rng, len(s) + 1 + i % 3) for i, s in enumerate(seqs)]           # as many reads, other lengths
    reads, reads_other = ctx.reads_from_ascii(seqs), ctx.reads_from_ascii(other)
    sp = ctx.kminmer_spans(reads, scan(ctx, reads, 13, 0.1, True), K=13, hpc=True, k=4)
    sp_other = ctx.kminmer_spans(reads_other, scan(ctx, reads_other, 13, 0.1, True), K=13, hpc=True, k=4)
    spans = sp.to_host()
    n_win = sp.info()["n_windows"]
    good_w, good_p = np.arange(0, n_win, 3), np.arange(0, n_win, 3) % 3
    want = EM.expected_requests(seqs, spans, good_w, good_p, EM.BITSET)
    SENTINEL = 0x5A5A5A5A

    def outcome(rc, out_h, names):
        assert rc == -1, rc                                                           # MDBG_EINVAL
        assert out_h.value == SENTINEL
        msg = (L.mdbg_last_error(ctx.h) or b"").decode()
        if names is not None:
            assert f"request {names}:" in msg, msg
        EM.assert_equal(ctx.spans_extract(reads, sp, good_w, good_p).to_host(), want, "a correct call behind a refusal")

    def refused_request(at, window, part, reserved=0, form=capi.SEQ_BITSET, reads_h=None, spans_h=None, names=True):
        req = np.zeros(len(good_w), capi.SEQ_REQUEST)
        req["window"], req["part"] = good_w, good_p
        req[at] = (window, part, reserved)
        out_h = C.c_void_p(SENTINEL)
        rc = L.mdbg_spans_extract(ctx.h, reads_h or reads.h, spans_h or sp.h, req.ctypes.data_as(C.c_void_p), len(req), form, C.byref(out_h))
        outcome(rc, out_h, at if names else None)

    def refused_range(at, rd, start, length, form=capi.SEQ_BITSET):
        rg = np.zeros(40, capi.SEQ_RANGE)
        rg["length"] = 10
        rg[at] = (rd, start, length, 0)
        out_h = C.c_void_p(SENTINEL)
        rc = L.mdbg_reads_extract_ranges(ctx.h, reads.h, rg.ctypes.data_as(C.c_void_p), len(rg), form, C.byref(out_h))
        outcome(rc, out_h, at)

    refused_request(5, n_win, 0)                                     # a window index equal to n_windows
    refused_request(7, 3, 3)                                         # part = 3
    refused_request(9, 3, 1, reserved=1)                             # non-zero reserved
    refused_request(len(good_w) - 1, 3, 3)                           # ... in the last request; and the FIRST offending one is named
    refused_range(11, 2, len(seqs[2]) - 9, 10)                       # a range one base too long
    refused_range(0, 2, 0xFFFFFFFF, 2)                               # start + length wraps 32 bits
    refused_range(13, len(seqs), 0, 1)                               # a read index equal to n_reads
    refused_request(0, 0, 0, form=2, names=False)                    # form out of range
    refused_request(0, 0, 0, spans_h=sp_other.h)                     # spans of another batch: as many reads, other lengths
    fewer = ctx.reads_from_ascii(seqs[:-1])
    refused_request(0, 0, 0, reads_h=fewer.h, names=False)           # ... another number of reads
    # two offending requests: the first is named
    req = np.zeros(30, capi.SEQ_REQUEST)
    req[20] = (0, 7, 0)
    req[4] = (n_win + 5, 0, 0)
    out_h = C.c_void_p(SENTINEL)
    outcome(L.mdbg_spans_extract(ctx.h, reads.h, sp.h, req.ctypes.data_as(C.c_void_p), len(req), 0, C.byref(out_h)), out_h, 4)
    # null arguments
    out_h = C.c_void_p(SENTINEL)
    assert L.mdbg_spans_extract(ctx.h, None, sp.h, req.ctypes.data_as(C.c_void_p), 1, 0, C.byref(out_h)) == -1 and out_h.value == SENTINEL
    assert L.mdbg_spans_extract(ctx.h, reads.h, sp.h, None, 1, 0, C.byref(out_h)) == -1 and out_h.value == SENTINEL
    assert L.mdbg_reads_extract_ranges(ctx.h, reads.h, None, 1, 0, C.byref(out_h)) == -1 and out_h.value == SENTINEL
    assert L.mdbg_spans_extract(ctx.h, reads.h, sp.h, req.ctypes.data_as(C.c_void_p), 1, 0, None) == -1
    assert L.mdbg_sequences_info(None, None, None, None, None) == -1 and L.mdbg_sequences_device_ptrs(None, None, None, None) == -1
    assert L.mdbg_sequences_to_host(ctx.h, None, None, None, None) == -1
    L.mdbg_sequences_free(None)


# ---- 6. contexts, pool reuse, pointers, timers ---------------------------------------------------------------------------------------
def test_two_contexts_alternating_and_a_second_call(ctx):
    """A second call on a context takes its buffers from the pool the first call's went back to (characters, then the smaller bitset in the
    same block): padding still zero.  Two contexts take turns on their own reads."""
    rng = np.random.default_rng(81)
    other = capi.Context(0)
    try:
        sides = []
        for c in (ctx, other):
            seqs = [rand_seq(rng, int(n)) for n in rng.integers(100, 4000, 40)]
            rd = rng.integers(0, len(seqs), 700)
            ln = np.array([rng.integers(0, min(len(seqs[r]), 333) + 1) for r in rd], dtype=np.int64)
            st = np.array([rng.integers(0, len(seqs[r]) - l + 1) for r, l in zip(rd, ln)], dtype=np.int64)
            sides.append((c, seqs, c.reads_from_ascii(seqs), np.stack([rd, st, ln, rng.integers(0, 2, 700)], axis=1)))
        for turn in range(3):
            for c, seqs, reads, rg in sides:
                for form in (capi.SEQ_ASCII, capi.SEQ_BITSET, capi.SEQ_BITSET):
                    cut = rg[turn * 100:]
                    EM.assert_equal(extract_ranges(c, reads, cut, form), EM.expected(seqs, cut[:, 0], cut[:, 1], cut[:, 2], cut[:, 3], form), f"turn {turn}")
    finally:
        other.close()


def test_device_pointers_and_timers(ctx, plain_batch):
    seqs, reads = plain_batch
    rg = np.array([(0, 5, 1000, 0), (0, 7, 1000, 1), (3, 0, 31, 0)])
    ctx.timing(True)
    ctx.timing_reset()
    try:
        sq = ctx.reads_extract_ranges(reads, rg[:, 0], rg[:, 1], rg[:, 2], rg[:, 3], capi.SEQ_BITSET)
        ctx.synchronize()
        assert ctx.timing_get("extract_plan")[1] == 1 and ctx.timing_get("extract_copy")[1] == 1
    finally:
        ctx.timing(False)
    got = sq.to_host()
    p = sq.device_ptrs()
    assert all(p.values()) and len(set(p.values())) == 3 and p["bytes"] % 8 == 0
    # the device arrays are what mdbg_sequences_to_host copies: a device-to-device copy of one sequence over another shows in the next download
    assert list(got["byte_offsets"]) == [0, 256, 512, 520] and got["bytes"][:250].tobytes() != got["bytes"][256:506].tobytes()
    ctx.memcpy_device(p["bytes"] + 256, p["bytes"], 256)
    again = sq.to_host()["bytes"]
    assert again[256:512].tobytes() == got["bytes"][:256].tobytes()
    for name in ("extract_plan", "extract_plan_ranges", "extract_copy"):
        a = ctx.kernel_attributes(name)
        assert a["scratch"] == 0 and a["static_lds"] == 0, (name, a)
    sq.close()
