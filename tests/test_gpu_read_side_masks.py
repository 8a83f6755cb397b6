"""The three kernels that build a read batch on the device -- pack_ascii_kernel (mdbg_reads_from_ascii), mask_listed_kernel
(mdbg_reads_mark_ascii on a packed batch: the host feed's path) and fastx_pack_kernel (mdbg_reads_from_fastx_bytes) -- bit for bit against
tests/reads_model.py: every array of Reads.packed_to_host() and every field of its info, on inputs that put every ordered pair of
characters on every bit of a word, odd characters in the first and last base of reads at every word-count border, changes across word
borders and across base 2048 (word 64: a lane's second trip), and more reads than the grid has waves.  Then the scan at the same seams
against the oracle, at densities where a wrong mask bit cannot hide (tests/test_reads_model.py proves that per case)."""
from __future__ import annotations

import numpy as np
import pytest

from metamdbg_amd import formats, synth
from tests import reads_model as M

pytestmark = pytest.mark.gpu

ARRAYS = ("word_offsets", "lengths", "words", "invalid", "breaks", "masked", "masked_list")
FIELDS = ("has_invalid", "has_break", "n_masked", "n_words")
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4097)


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def plain(rng, n: int) -> bytes:
    return synth.CODE2ASCII[rng.integers(0, 4, n)].tobytes()


def pair_reads(rng):
    """All 256 ordered pairs of neighbours behind 0 .. 31 plain bases: every pair on every bit of a word, bit 0 included."""
    s = M.all_pairs()
    return [plain(rng, front) + s for front in range(32)]


def length_reads(rng):
    """Every length at which the word count, the tail word or the lane trip changes, with an odd character in its first base and in its
    last, each of which carries a bit: an invalid character in the first base (base 0 never breaks); in the last base an invalid
    character or, from read to read, the lower case of the base before it -- a break bit on the read's last bit."""
    invalid = b"NnKMY"
    out = []
    for j, L in enumerate(LENGTHS):
        s = bytearray(plain(rng, L))
        if L:
            s[0] = invalid[j % 5]
            if j % 2 and L >= 3:
                s[L - 1] = s[L - 2] + 32
            else:
                s[L - 1] = invalid[(j + 2) % 5]
        out.append(bytes(s))
    return out


def seam_reads(rng):
    """A change of character across a word border, across the border of the lane's trips (base 2048) and across 4095 | 4096."""
    out = []
    for at in (32, 64, 2048, 4096):
        for pair in (b"aA", b"Cc", b"NG", b"KM"):
            s = bytearray(plain(rng, at + 100))
            s[at - 1:at + 1] = pair
            out.append(bytes(s))
    return out


def grid_reads(rng, n_cu: int):
    """More reads than the producers' grids have waves (n_cu * 16 workgroups of four): the grid-stride loop takes a second trip."""
    alphabet = np.frombuffer(M.ALPHABET, np.uint8)
    out = []
    for j, L in enumerate(rng.integers(0, 71, n_cu * 64 + 77)):
        out.append(alphabet[rng.integers(0, 16, int(L))].tobytes() if j % 10 == 3 else plain(rng, int(L)))
    out[-1] = b"GATTACAn"                       # the last read of the second trip is odd in its last base
    return out


@pytest.fixture(scope="module")
def batches(ctx):
    """name -> (reads, model): built once and left alone."""
    rng = np.random.default_rng(77)
    b = dict(pairs=pair_reads(rng), lengths=length_reads(rng), seams=seam_reads(rng), grid=grid_reads(rng, ctx.device_info()["n_cu"]),
             plain=[plain(rng, n) for n in (200, 0, 64, 33, 2049)],
             lower_only=[plain(rng, 100), b"ACGTacgtaAcCgGtT" * 5, plain(rng, 70).lower() + b"aA"],
             n_only=[plain(rng, 50), b"ACGT" + b"N" * 40 + b"ACGTT", b"NNNN", plain(rng, 2047) + b"NN" + plain(rng, 10)])
    return {k: (v, M.pack(v)) for k, v in b.items()}


def assert_same(got: dict, want: dict, what, words: bool = True):
    for k in FIELDS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ARRAYS:
        if k == "words" and not words:
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        if not np.array_equal(got[k], want[k]):
            at = int(np.flatnonzero(got[k] != want[k])[0])
            raise AssertionError(f"{what}: {k}[{at}] is {int(got[k][at]):#x}, the model says {int(want[k][at]):#x}")


def test_flag_states_of_the_model(batches):
    """What the three flag-state batches are meant to be, by the model: the producers below are then held to it."""
    p, lo, n = batches["plain"][1], batches["lower_only"][1], batches["n_only"][1]
    assert not p["has_invalid"] and not p["has_break"] and p["n_masked"] == 0
    assert lo["has_invalid"] and lo["has_break"] and not lo["invalid"].any() and lo["masked"].tolist() == [0, 1, 1]
    assert n["has_invalid"] and not n["has_break"] and n["masked"].tolist() == [0, 1, 1, 1]
    g = batches["grid"][1]
    assert 0 < g["n_masked"] < len(g["masked"]) // 5 and g["masked"][-1] == 1


@pytest.mark.parametrize("name", ["pairs", "lengths", "seams", "grid", "plain", "lower_only", "n_only"])
def test_reads_from_ascii(ctx, batches, name):
    seqs, want = batches[name]
    reads = ctx.reads_from_ascii(seqs)
    assert_same(reads.packed_to_host(), want, name)
    assert reads.info() == dict(n_reads=len(seqs), n_bases=sum(map(len, seqs)), n_words=want["n_words"])
    reads.free()


def packed(seqs):
    words, woff, lens = synth.pack_reads([synth.ascii_to_codes(s) for s in seqs])
    return np.ascontiguousarray(words, np.uint64), np.ascontiguousarray(woff, np.uint64), np.ascontiguousarray(lens, np.uint32)


def listings(seqs):
    """The three ways a feeder may list reads: exactly the odd ones; the odd ones and some plain ones (every read, in fact: the listed
    kernel's grid stride needs more listed reads than waves); half of the odd ones -- the others then have zero masks by contract."""
    odd = [r for r, s in enumerate(seqs) if M.is_odd(s)]
    return dict(odd=odd, all=list(range(len(seqs))), half=odd[::2])


@pytest.mark.parametrize("name", ["pairs", "lengths", "seams", "grid", "plain", "lower_only", "n_only"])
def test_packed_upload_then_mark_ascii(ctx, batches, name):
    seqs, full = batches[name]
    words, woff, lens = packed(seqs)
    for how, listed in listings(seqs).items():
        want = full if how != "half" else M.mark(seqs, listed)
        if how == "odd":                         # a read with no bit is plain, and a plain read has no bit: listing the odd reads loses nothing
            assert np.array_equal(M.mark(seqs, listed)["masked"], full["masked"])
        reads = ctx.reads_from_packed(words, woff, lens)
        before = reads.packed_to_host()          # never marked: no masks, the caller's words as they are
        assert not before["has_invalid"] and not before["has_break"] and before["n_masked"] == 0 and len(before["masked_list"]) == 0
        assert not before["invalid"].any() and not before["breaks"].any() and not before["masked"].any() and np.array_equal(before["words"], words)
        reads.mark_ascii(listed, [seqs[r] for r in listed])
        got = reads.packed_to_host()
        assert_same(got, want, (name, how), words=False)
        assert np.array_equal(got["words"], words)
        assert set(got["masked_list"].tolist()) <= set(r for r in listed if M.is_odd(seqs[r]))         # a listed plain read is not in the list
        reads.free()


@pytest.mark.parametrize("name", ["pairs", "lengths", "seams", "grid", "plain", "lower_only", "n_only"])
def test_async_packed_upload_marked_before_the_wait(ctx, batches, name):
    seqs, want = batches[name]
    words, woff, lens = packed(seqs)
    reads = ctx.reads_from_packed_async(words, woff, lens)
    odd = [r for r, s in enumerate(seqs) if M.is_odd(s)]
    reads.mark_ascii(odd, [seqs[r] for r in odd])
    got = reads.packed_to_host()                 # (waits for the upload itself)
    reads.wait()
    assert_same(got, want, name, words=False)
    assert np.array_equal(got["words"], words)
    reads.free()


def fasta(seqs, width, eol):
    out = []
    for i, s in enumerate(seqs):
        out.append(b">r%d" % i + eol)
        for at in range(0, len(s), width or max(1, len(s))):
            out.append(s[at:at + (width or len(s))] + eol)
    return b"".join(out)


def fastq(seqs, eol):
    return b"".join(b"@r%d" % i + eol + s + eol + b"+" + eol + b"I" * len(s) + eol for i, s in enumerate(seqs))


def check_fastx(ctx, text, want, what):
    b = ctx.bytes_from_host(text)
    reads = ctx.reads_from_fastx_bytes(b)
    assert_same(reads.packed_to_host(), want, what)
    assert reads.fastx_info["n_masked"] == want["n_masked"] and reads.fastx_info["n_reads"] == len(want["lengths"])
    reads.free()
    b.free()


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
@pytest.mark.parametrize("width", [60, 61, None])
def test_reads_from_fasta_bytes(ctx, batches, width, eol):
    """(grid: reads of up to 70 bases, so widths 60 and 61 wrap reads of the grid-stride loop's second trip too)"""
    for name in ("pairs", "lengths", "seams", "grid", "plain", "lower_only", "n_only"):
        seqs, want = batches[name]
        check_fastx(ctx, fasta(seqs, width, eol), want, (name, width, eol))


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
def test_reads_from_fastq_bytes(ctx, batches, eol):
    for name in ("pairs", "lengths", "seams", "grid", "plain", "lower_only", "n_only"):
        seqs, want = batches[name]
        check_fastx(ctx, fastq(seqs, eol), want, (name, eol))


# ---- the scan at the same seams, against the oracle ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def records(orc, seqs, density, hpc):
    return [orc.read_selection(s, None, K=M.SEAM_K, density=density, hpc=hpc)["record"] for s in seqs]


def scan_records(ctx, seqs, density, hpc) -> bytes:
    reads = ctx.reads_from_ascii(seqs)
    m = ctx.scan(reads, K=M.SEAM_K, density=density, hpc=hpc)
    got = formats.build_read_data_init(m.to_host())
    m.free()
    reads.free()
    return got


def block_launches(ctx) -> int:
    info = ctx.scan_info()
    return info["prefiltered_launches"] + info["block_launches"]


@pytest.mark.parametrize("hpc", [True, False])
def test_scan_at_mask_seams_every_kmer_visible(ctx, orc, hpc):
    """Density 1.0: the general kernel, and every k-mer that a mask bit touches is in the output -- those that touch an invalid character
    too, as 0xFFFFFFFF: the reference gives them the value -1 and hashes it like any other (Kmer.hpp:567, :580, :1434), which selects them
    at densities above 0.7135.  (The N at base 1 showed that the kernel dropped them at every density.)"""
    seqs = [c["seq"] for c in M.seam_cases(1.0, hpc)]
    before = block_launches(ctx)
    assert scan_records(ctx, seqs, 1.0, hpc) == b"".join(records(orc, seqs, 1.0, hpc))
    assert block_launches(ctx) == before


@pytest.mark.parametrize("hpc", [True, False])
def test_scan_at_mask_seams_without_end_trim(ctx, orc, hpc):
    """The same reads with MinimizerParser::_trimBps = 0 (mdbg_scan_params::no_end_trim), against the oracle's untrimmed parser: value,
    position and direction of every k-mer, the read's first and its last included.  The last one is written by a branch of its own in the
    kernel (no base follows it); in the reads with an N or K in their last K bases it touches an invalid character and is 0xFFFFFFFF."""
    seqs = [c["seq"] for c in M.seam_cases(1.0, hpc)]
    reads = ctx.reads_from_ascii(seqs)
    m = ctx.scan(reads, K=M.SEAM_K, density=1.0, hpc=hpc, apply_read_filters=False, no_end_trim=True)
    h = m.to_host()
    m.free()
    reads.free()
    last_invalid = first_invalid = 0
    for i, s in enumerate(seqs):
        want = list(zip(*orc.minimizer_parse(s, M.SEAM_K, 1.0, hpc, trim=0)))
        a, b = int(h["offsets"][i]), int(h["offsets"][i + 1])
        got = list(zip(h["minimizers"][a:b].tolist(), h["pos"][a:b].tolist(), h["dir"][a:b].tolist()))
        assert got == want, (i, M.seam_cases(1.0, hpc)[i]["p"], M.seam_cases(1.0, hpc)[i]["kind"])
        last_invalid += want[-1][0] == 0xFFFFFFFF
        first_invalid += want[0][0] == 0xFFFFFFFF
    assert last_invalid >= 6 and first_invalid >= 6        # N and K at bases L-K, L-2 and L-1; at bases 0, 1 and K-1


@pytest.mark.parametrize("hpc", [True, False])
def test_scan_at_mask_seams_every_read_odd(ctx, orc, hpc):
    """Density 0.19 is below the block path's limit, but with every read masked (n_masked * 8 > n + 128) the batch is not routed: the
    general kernel scans it all, and neither block kernel is launched."""
    seqs = [c["seq"] for c in M.seam_cases(0.19, hpc)]
    assert len(seqs) * 8 > len(seqs) + 128
    before = block_launches(ctx)
    assert scan_records(ctx, seqs, 0.19, hpc) == b"".join(records(orc, seqs, 0.19, hpc))
    assert block_launches(ctx) == before


@pytest.mark.parametrize("hpc", [True, False])
def test_scan_at_mask_seams_routed(ctx, orc, hpc):
    """16 odd reads among 200 plain ones: the block-structured kernel scans the plain reads and skips the odd ones, which the general
    kernel finishes.  The plain reads are 1000 bases, so that the batch's average read is expected to fit the block kernel's stage of 384
    rows at this density ((16 * 2300 + 200 * 1000) / 216 = 1096 bases; 1096 * 0.19 * 1.4 + 24 = 316 rows) and the batch takes that path."""
    rng = np.random.default_rng(5)
    plain_reads = [plain(rng, 1000) for _ in range(200)]
    plain_records = records(orc, plain_reads, 0.19, hpc)
    cases = M.seam_cases(0.19, hpc)
    for first in range(0, len(cases), 16):
        odd = [c["seq"] for c in cases[first:first + 16]]
        slots = sorted(rng.choice(200 + len(odd), len(odd), replace=False).tolist())
        seqs, want = list(plain_reads), list(plain_records)
        for at, s, rec in zip(slots, odd, records(orc, odd, 0.19, hpc)):
            seqs.insert(at, s)
            want.insert(at, rec)
        before = block_launches(ctx)
        assert scan_records(ctx, seqs, 0.19, hpc) == b"".join(want), first
        assert block_launches(ctx) > before, first
