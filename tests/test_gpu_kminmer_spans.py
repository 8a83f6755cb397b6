"""mdbg_kminmer_spans (csrc/spans.hip, csrc/spans_dev.hpp): per window of k minimizers its identity and the ReadKminmer fields of
MDBG::getKminmers (Commons.hpp:5401-5526) in the ORIGINAL read's coordinates, from the reads and their scan, on the device.  Expected
values: the reference's own answers under tests/golden/kminmer_spans (written by the generator committed there) and a numpy restatement
of the formulas (tests/spans_model.py: EncoderRLE::execute's map over the characters, the identity from pyoracle.kminmer_normalize_hash).
The restatement was compared against the fixture on the CPU.
Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import pytest

from metamdbg_amd import capi, synth
from tests import helpers as H
from tests import spans_model as SM

pytestmark = pytest.mark.gpu

FIX = os.path.join(H.GOLDEN, "kminmer_spans")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def rand_seq(rng, n: int, runs: bool = True) -> bytes:
    """Seeded ACGT; runs = False: no two equal neighbours (L' = L)."""
    if runs:
        return bytes(synth.CODE2ASCII[rng.integers(0, 4, int(n))])
    c = np.zeros(int(n), dtype=np.int64)
    if n:
        c[0] = rng.integers(0, 4)
        c[1:] = rng.integers(1, 4, int(n) - 1)
    return bytes(synth.CODE2ASCII[np.cumsum(c) % 4])


def revcomp(s: bytes) -> bytes:
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def scan(ctx, reads, l, density, hpc, no_end_trim=False):
    return ctx.scan(reads, K=l, density=density, hpc=hpc, apply_read_filters=False, no_end_trim=no_end_trim)


def spans_and_expected(ctx, seqs, l, density, hpc, k, no_end_trim=False, reads=None):
    """(what the library returns, what the restatement expects from the same scan, the scan on the host)."""
    reads = reads if reads is not None else ctx.reads_from_ascii(seqs)
    mins = scan(ctx, reads, l, density, hpc, no_end_trim)
    got = ctx.kminmer_spans(reads, mins, K=l, hpc=hpc, k=k).to_host()
    h = mins.to_host()
    assert np.array_equal(h["read_length"], [len(s) for s in seqs])
    return got, SM.expected(seqs, h["offsets"], h["minimizers"], h["pos"], l, hpc, k), h


# ---- 1. the reference's answers ------------------------------------------------------------------------------------------------------
with open(os.path.join(FIX, "manifest.json")) as _f:
    MANIFEST = json.load(_f)


@pytest.fixture(scope="module")
def fixture_reads():
    with open(os.path.join(FIX, MANIFEST["reads"]), "rb") as f:
        reads = f.read().split(b"\n")[:-1]
    assert len(reads) == MANIFEST["n_reads"] and sum(len(r) > 3000 for r in reads) == 1 and max(map(len, reads)) == 70_000
    return reads


@pytest.mark.parametrize("cfg", MANIFEST["configs"], ids=[c["name"] for c in MANIFEST["configs"]])
def test_fixture_from_the_reference(ctx, fixture_reads, cfg):
    """reads -> mdbg_reads_from_ascii -> mdbg_scan -> mdbg_kminmer_spans against EncoderRLE + MinimizerParser + MDBG::getKminmers: every array
    equal.  (l 15, compression, k 4), (15, compression, 13), (13, compression, no end trim, density 1.0, k 2: every position selected, the
    last minimizer of a read ends at the sentinel rle[L']), (15, no compression, k 5)."""
    want = np.load(os.path.join(FIX, cfg["name"] + ".npz"))
    seqs = [fixture_reads[i] for i in cfg["reads"]]
    reads = ctx.reads_from_ascii(seqs)
    mins = scan(ctx, reads, cfg["l"], cfg["density"], bool(cfg["hpc"]), no_end_trim=cfg["trim"] == 0)
    sp = ctx.kminmer_spans(reads, mins, K=cfg["l"], hpc=bool(cfg["hpc"]), k=cfg["k"])
    assert sp.info() == dict(n_reads=len(seqs), n_minimizers=cfg["n_minimizers"], n_windows=cfg["n_windows"], k=cfg["k"])
    got = sp.to_host()
    h = mins.to_host()
    for f in ("offsets", "minimizers", "pos"):
        assert np.array_equal(h[f], want[f]), f
    SM.assert_equal(got, want, cfg["name"])
    assert np.array_equal(got["pos_end"] - got["pos_start"], want["length"])         # _length
    assert 0 < cfg["n_reversed"] < cfg["n_windows"] and int(got["reversed"].sum()) == cfg["n_reversed"]
    if cfg["density"] == 1.0:
        last = h["offsets"][1:][np.diff(h["offsets"].astype(np.int64)) > 0].astype(np.int64) - 1
        assert len(last) > 10 and np.array_equal(got["min_end"][last], h["read_length"][np.diff(h["offsets"].astype(np.int64)) > 0])


# ---- 2. homopolymer geometry ---------------------------------------------------------------------------------------------------------
def geometry_reads(l: int) -> list[bytes]:
    rng = np.random.default_rng(5)

    def with_run(at: int, run: int, tail: int) -> bytes:
        a, b = bytearray(rand_seq(rng, at)), bytearray(rand_seq(rng, tail))
        if a and a[-1] == ord("G"):
            a[-1] = ord("T")
        if b and b[0] == ord("G"):
            b[0] = ord("C")
        return bytes(a) + b"G" * run + bytes(b)

    seqs = [with_run(at, run, 150) for at in (28, 31, 60, 63, 2040, 2047) for run in (2, 9, 40)]   # across a 32-base word, a 64-base and the 2048-base tile border
    seqs += [with_run(700, 5000, 900), with_run(2048 * 3 - 20, 5000, 30)]                           # a run of 5000: words and whole tiles without a run start
    seqs += [b"A" * 1, b"C" * 77, b"T" * 2048, b"G" * 2100]                                        # one run: L' = 1, no minimizer
    seqs += [rand_seq(rng, n, runs=False) for n in (1, l - 1, l, l + 1)]
    seqs += [with_run(end - 11, 11, 0) for end in (32, 64, 2048, 4096)]                            # the last run ends exactly on a word border
    seqs += [rand_seq(rng, n) for n in (2047, 2048, 2049, 4500)]
    return seqs


def test_homopolymer_geometry_every_span_of_every_read(ctx):
    """Density 1.0 and no end trim: every compressed position p in 0 .. L' - l is a minimizer, so every S = rle[p] and every E = rle[p + l] of
    the read is compared, the sentinel E = length included."""
    l = 13
    seqs = geometry_reads(l)
    got, want, h = spans_and_expected(ctx, seqs, l, 1.0, True, 2, no_end_trim=True)
    n = np.diff(h["offsets"].astype(np.int64))
    for r, s in enumerate(seqs):
        lc = len(SM.rle_positions(s, True)) - 1
        assert n[r] == max(0, lc - l + 1), (r, len(s), lc)                     # every position was selected ...
    assert (n[-12:-8] == [0, 0, 1, 2]).all()                                  # ... lengths 1, l - 1, l, l + 1
    assert (n[20:24] == 0).all()
    SM.assert_equal(got, want, "geometry")
    has = n > 0
    assert np.array_equal(got["min_end"][h["offsets"][1:][has].astype(np.int64) - 1], h["read_length"][has])     # E = length
    assert np.array_equal(got["window_offsets"], np.concatenate([[0], np.cumsum(np.maximum(n - 1, 0))]))


def test_without_compression_the_map_is_the_identity(ctx):
    l = 15
    seqs = geometry_reads(l)
    got, want, h = spans_and_expected(ctx, seqs, l, 0.2, False, 3)
    SM.assert_equal(got, want, "no compression")
    assert np.array_equal(got["min_start"], h["pos"]) and np.array_equal(got["min_end"], h["pos"] + l)


# ---- 3. characters -------------------------------------------------------------------------------------------------------------------
def test_characters_ascii_and_packed_marked(ctx):
    """N runs, "aA", IUPAC letters that share a code, an N next to a G: a change of character starts a run although the 2-bit codes agree.  The
    same reads through mdbg_reads_from_ascii and through mdbg_reads_from_packed + mdbg_reads_mark_ascii."""
    rng = np.random.default_rng(9)
    body = lambda n: rand_seq(rng, n)
    seqs = [body(300), body(40) + b"N" * 50 + body(200) + b"NNN" + body(100), body(31) + b"aA" * 20 + body(120) + b"AaAAaa" + body(64),
            body(100) + b"CSCSSc" + body(90) + b"GRrRK" + body(77) + b"TtYyWw" + body(50), body(50) + b"GNG" + body(61) + b"NGGN" + body(200) + b"gNnG" + body(30),
            body(2040) + b"GGGGNNNNNNGGGG" + body(300), b"N" + body(150), body(150) + b"N", body(500)]
    odd = [1, 2, 3, 4, 5, 6, 7]
    l = 13
    for hpc, density, trim0, k in ((True, 1.0, True, 2), (True, 0.3, False, 4), (False, 0.3, False, 3)):
        got, want, h = spans_and_expected(ctx, seqs, l, density, hpc, k, no_end_trim=trim0)
        SM.assert_equal(got, want, f"characters hpc {hpc}")
        assert len(got["reversed"]) > 100
        words, woff, lens = synth.pack_reads([synth.ascii_to_codes(x) for x in seqs])
        reads = ctx.reads_from_packed(words, woff, lens)
        reads.mark_ascii(odd, [seqs[r] for r in odd])
        got2, want2, h2 = spans_and_expected(ctx, seqs, l, density, hpc, k, no_end_trim=trim0, reads=reads)
        assert np.array_equal(h2["pos"], h["pos"]) and np.array_equal(h2["minimizers"], h["minimizers"])
        SM.assert_equal(got2, got, f"packed and marked, hpc {hpc}")


# ---- 4. windows ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def window_batch(ctx):
    """One batch for every k: seeded reads, reads made of a sequence followed by its reverse complement (their minimizer list is a palindrome:
    tie windows at its centre), and reads cut so that they hold k - 1, k and k + 1 minimizers for each k."""
    rng = np.random.default_rng(21)
    l, density = 13, 0.15
    base = [rand_seq(rng, int(n)) for n in rng.integers(200, 1500, 24)]
    half = [rand_seq(rng, int(n)) for n in (1500, 2500, 4000)]
    pal = [x + revcomp(x) for x in half]
    long_one = rand_seq(rng, 4000)
    probe = ctx.reads_from_ascii([long_one])
    hp = scan(ctx, probe, l, density, True).to_host()
    rle = SM.rle_positions(long_one, True)
    cuts = []
    for k in KS:
        for n in (k - 1, k, k + 1):              # the prefix that ends just behind minimizer n - 1, one base more so the end trim keeps it
            cuts.append(long_one[: int(rle[int(hp["pos"][n - 1]) + l + 1])])
    seqs = base + pal + cuts
    reads = ctx.reads_from_ascii(seqs)
    mins = scan(ctx, reads, l, density, True)
    return dict(seqs=seqs, reads=reads, mins=mins, l=l, n_base=len(base), n_pal=len(pal), h=None)


KS = (2, 4, 11, 12, 13, 33)


@pytest.mark.parametrize("k", KS)
def test_windows_for_every_form_of_the_hash(ctx, window_batch, k):
    """k = 2 (the second minimizer is the last), the specialised forms (4, 11) and the block-wise generic form (12, 13, 33: tails of 0, 1 and 1
    word behind 3, 3 and 8 blocks)."""
    b = window_batch
    got = ctx.kminmer_spans(b["reads"], b["mins"], K=b["l"], hpc=True, k=k).to_host()
    h = b["mins"].to_host()
    want = SM.expected(b["seqs"], h["offsets"], h["minimizers"], h["pos"], b["l"], True, k)
    SM.assert_equal(got, want, f"k {k}")
    n = np.diff(h["offsets"].astype(np.int64))
    assert np.array_equal(got["window_offsets"], np.concatenate([[0], np.cumsum(np.maximum(n - k + 1, 0))]))
    at = b["n_base"] + b["n_pal"] + 3 * KS.index(k)
    assert list(n[at:at + 3]) == [k - 1, k, k + 1]                                  # reads with n = k - 1, k, k + 1 minimizers ...
    assert list(np.diff(got["window_offsets"].astype(np.int64))[at:at + 3]) == [0, 1, 2]      # ... hold 0, 1 and 2 windows
    # a palindromic read: its minimizer list reads the same backwards, so the window at its centre ties (even k) and is reversed
    ties = 0
    for r in range(b["n_base"], b["n_base"] + b["n_pal"]):
        m = h["minimizers"][int(h["offsets"][r]):int(h["offsets"][r + 1])]
        assert np.array_equal(m, m[::-1]) and len(m) >= 40 and len(m) % 2 == 0
        for w in range(len(m) - k + 1):
            if np.array_equal(m[w:w + k], m[w:w + k][::-1]):
                ties += 1
                assert got["reversed"][int(got["window_offsets"][r]) + w] == 1
    assert ties >= (3 if k % 2 == 0 else 0)
    assert 0 < got["reversed"].sum() < len(got["reversed"])


# ---- 5. forms of the input -----------------------------------------------------------------------------------------------------------
def test_fresh_scan_output_and_canonical(ctx):
    rng = np.random.default_rng(31)
    seqs = [rand_seq(rng, int(n)) for n in rng.integers(500, 9000, 300)]
    reads = ctx.reads_from_ascii(seqs)
    mins = scan(ctx, reads, 15, 0.02, True)                     # fresh: in the order the waves finished
    first = ctx.kminmer_spans(reads, mins, K=15, hpc=True, k=4).to_host()
    h = mins.to_host()                                          # canonical now
    again = ctx.kminmer_spans(reads, mins, K=15, hpc=True, k=4).to_host()
    SM.assert_equal(first, again, "fresh against canonical")
    SM.assert_equal(first, SM.expected(seqs, h["offsets"], h["minimizers"], h["pos"], 15, True, 4), "fresh scan output")


def test_fastq_reads(ctx):
    rng = np.random.default_rng(33)
    seqs = [rand_seq(rng, int(n)) for n in rng.integers(100, 5000, 60)]
    quals = [bytes(rng.integers(35, 75, len(s)).astype(np.uint8)) for s in seqs]
    reads = ctx.reads_from_ascii(seqs, quals)
    got, want, _ = spans_and_expected(ctx, seqs, 15, 0.05, True, 5, reads=reads)
    SM.assert_equal(got, want, "reads with qualities")
    assert len(got["reversed"]) > 500


def test_concat_of_two_scans_against_the_reads_as_one(ctx):
    rng = np.random.default_rng(35)
    a = [rand_seq(rng, int(n)) for n in rng.integers(100, 4000, 40)]
    b = [rand_seq(rng, int(n)) for n in rng.integers(100, 4000, 25)]
    ma, mb = scan(ctx, ctx.reads_from_ascii(a), 15, 0.05, True), scan(ctx, ctx.reads_from_ascii(b), 15, 0.05, True)
    both = ctx.minimizers_concat([ma, mb])
    reads = ctx.reads_from_ascii(a + b)
    got = ctx.kminmer_spans(reads, both, K=15, hpc=True, k=4).to_host()
    h = both.to_host()
    SM.assert_equal(got, SM.expected(a + b, h["offsets"], h["minimizers"], h["pos"], 15, True, 4), "concat")
    whole = ctx.kminmer_spans(reads, scan(ctx, reads, 15, 0.05, True), K=15, hpc=True, k=4).to_host()
    SM.assert_equal(got, whole, "concat against one scan")


def test_long_reads_whole_and_in_segments(ctx):
    """A read of about 70 kb and one of 300 kb among 64 short ones, scanned whole ("scan_segments" 0) and cut into segments (2): the map does
    not depend on a read's length, and both scans give the same spans."""
    rng = np.random.default_rng(37)
    seqs = [rand_seq(rng, int(n)) for n in rng.integers(500, 6000, 64)]
    seqs.insert(10, rand_seq(rng, 70_123))
    seqs.insert(40, rand_seq(rng, 300_001))
    reads = ctx.reads_from_ascii(seqs)
    out = []
    try:
        for seg in (0, 2):
            ctx.set_option("scan_segments", seg)
            mins = scan(ctx, reads, 15, 0.005, True)
            out.append((ctx.kminmer_spans(reads, mins, K=15, hpc=True, k=4).to_host(), mins.to_host()))
    finally:
        ctx.set_option("scan_segments", -1)
    SM.assert_equal(out[0][0], out[1][0], "whole against segments")
    h = out[0][1]
    SM.assert_equal(out[0][0], SM.expected(seqs, h["offsets"], h["minimizers"], h["pos"], 15, True, 4), "long reads")
    n = np.diff(h["offsets"].astype(np.int64))
    assert n[10] > 150 and n[40] > 800


def test_zero_reads_and_zero_windows(ctx):
    empty = ctx.reads_from_ascii([])
    got = ctx.kminmer_spans(empty, scan(ctx, empty, 15, 0.005, True), K=15, hpc=True, k=4).to_host()
    assert list(got["window_offsets"]) == [0] and all(len(got[f]) == 0 for f in SM.FIELDS[1:])
    rng = np.random.default_rng(39)
    seqs = [rand_seq(rng, 40), b"", rand_seq(rng, 10)]
    got, want, h = spans_and_expected(ctx, seqs, 15, 1.0, True, 33, no_end_trim=True)
    assert len(h["minimizers"]) > 0 and list(got["window_offsets"]) == [0, 0, 0, 0] and len(got["hash_lo"]) == 0
    SM.assert_equal(got, want, "zero windows")


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_by_argument_checks(ctx):
    """Each is MDBG_EINVAL, *out stays untouched, and a correct call straight afterwards on the same context succeeds.  mdbg_kminmer_index sets
    no upper limit on k (a k above every read's count of minimizers gives an empty table), so neither does this call: zero windows."""
    L = capi.lib()
    rng = np.random.default_rng(41)
    seqs = [rand_seq(rng, int(n)) for n in rng.integers(300, 3000, 20)]
    other = [rand_seq(rng, len(s) + 1 + i % 3) for i, s in enumerate(seqs)]           # as many reads, other lengths
    reads, reads_other = ctx.reads_from_ascii(seqs), ctx.reads_from_ascii(other)
    mins = scan(ctx, reads, 13, 0.1, True)
    h = mins.to_host()
    want = SM.expected(seqs, h["offsets"], h["minimizers"], h["pos"], 13, True, 4)
    SENTINEL = 0x5A5A5A5A

    def refused(reads_h, mins_h, l, hpc, k, out=True, context=True, names=None):
        out_h = C.c_void_p(SENTINEL)
        rc = L.mdbg_kminmer_spans(ctx.h if context else None, reads_h, mins_h, l, int(hpc), k, C.byref(out_h) if out else None)
        assert rc == -1, rc                                                           # MDBG_EINVAL
        assert out_h.value == SENTINEL
        msg = (L.mdbg_last_error(ctx.h if context else None) or b"").decode()
        if names is not None:
            assert f"read {names}:" in msg, msg
        SM.assert_equal(ctx.kminmer_spans(reads, mins, K=13, hpc=True, k=4).to_host(), want, "a correct call behind a refusal")
        return msg

    from_host = ctx.minimizers_from_host(h["minimizers"], h["offsets"])
    refused(reads.h, from_host.h, 13, True, 4)                                        # no positions
    fewer = ctx.reads_from_ascii(seqs[:-1])
    refused(fewer.h, mins.h, 13, True, 4)                                             # n_reads differ
    refused(reads_other.h, mins.h, 13, True, 4, names=0)                              # same n_reads, other lengths
    # the same lengths, positions that do not fit: a larger minimizer_size than the scan's puts p + l behind L' where a read's last
    # minimizer sits less than 16 compressed bases in front of its end
    dense = scan(ctx, reads, 13, 1.0, True, no_end_trim=True)
    hd = dense.to_host()
    first_with = int(np.flatnonzero(np.diff(hd["offsets"].astype(np.int64)) > 0)[0])
    refused(reads.h, dense.h, 16, True, 4, names=first_with)
    refused(reads.h, mins.h, 13, True, 0)                                             # k = 0
    refused(reads.h, mins.h, 13, True, 1)                                             # k = 1
    refused(reads.h, mins.h, 0, True, 4)                                              # minimizer_size outside 1 .. 16
    refused(reads.h, mins.h, 17, True, 4)
    refused(None, mins.h, 13, True, 4)                                                # null arguments
    refused(reads.h, None, 13, True, 4)
    refused(reads.h, mins.h, 13, True, 4, out=False)
    refused(reads.h, mins.h, 13, True, 4, context=False)
    # k above every read's count: no limit, as in mdbg_kminmer_index -- zero windows
    top = ctx.kminmer_spans(reads, mins, K=13, hpc=True, k=0xFFFFFFFF)
    assert top.info()["n_windows"] == 0 and top.info()["k"] == 0xFFFFFFFF
    got = top.to_host()
    assert not got["window_offsets"].any() and np.array_equal(got["min_start"], want["min_start"]) and np.array_equal(got["min_end"], want["min_end"])
    # the other entry points with null handles
    assert L.mdbg_spans_info(None, None, None, None, None) == -1 and L.mdbg_spans_device_ptrs(None, None, None, None, None, None) == -1
    assert L.mdbg_spans_to_host(ctx.h, None, *([None] * 10)) == -1
    L.mdbg_spans_free(None)


def test_device_pointers_and_timers(ctx):
    """mdbg_spans_device_ptrs hands out the result's own arrays; the two timers count the map's two groups of launches and the windows' one."""
    rng = np.random.default_rng(43)
    seqs = [rand_seq(rng, int(n)) for n in rng.integers(300, 3000, 50)]
    reads = ctx.reads_from_ascii(seqs)
    mins = scan(ctx, reads, 15, 0.05, True)
    ctx.timing(True)
    ctx.timing_reset()
    try:
        sp = ctx.kminmer_spans(reads, mins, K=15, hpc=True, k=4)
        ctx.synchronize()
        assert ctx.timing_get("spans_map")[1] == 2 and ctx.timing_get("spans_windows")[1] == 1      # counts + selects, then the windows
    finally:
        ctx.timing(False)
    got = sp.to_host()
    p = sp.device_ptrs()
    assert all(p.values()) and len(set(p.values())) == 5
    # the device arrays are what mdbg_spans_to_host copies: a device-to-device copy of one over another shows in the next download
    assert not np.array_equal(got["hash_lo"], got["hash_hi"])
    ctx.memcpy_device(p["hash_hi"], p["hash_lo"], 8 * len(got["hash_lo"]))
    assert np.array_equal(sp.to_host()["hash_hi"], got["hash_lo"])
