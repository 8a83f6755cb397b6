"""mdbg_purge_palindromes (csrc/minimizers.hip) where it really drops minimizers.  The replay kernel re-derives
Commons::purgePalindrome (centre expansion, smallest window length of each parity) and sits behind a 16-lane suspect detector, a
one-thread-per-read fix kernel with an LDS path (reads of up to 96 minimizers) and a global-memory path, a `fixed` / `work` side
buffer, a gather, and two input layouts (CSR, the scattered rows of a fresh scan).  Real scan output of random DNA has next to no
palindromic window, so the inputs here are made to have them: small alphabets, planted palindromes, hairpin reads.

The expected value is always oracle.pyoracle.purge_palindrome read by read (the brute-force restatement of the reference's loop,
pinned to the reference's own outputs by fn_golden.json and fn/purge_long.json); the whole output is compared: values, offsets,
the object's count.  Every "this input exercises that path" claim is asserted on the ORACLE's answer, so an input that stops
exercising its path fails the test.  Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from metamdbg_amd import synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

LDS_MAX = 96        # PURGE_LDS_MAX of minimizers.hip: reads of up to 96 minimizers are replayed in LDS, longer ones in global memory


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _csr(lists):
    offs = np.zeros(len(lists) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in lists], out=offs[1:])
    mins = np.concatenate([np.asarray(x, dtype=np.uint32) for x in lists] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return mins, offs


def _assert_same(dev, mins, offs, what):
    """The whole output of a purge: values, offsets, and the count the object reports."""
    out = dev.to_host(full=False)
    assert dev.info()["n_minimizers"] == len(mins), what
    assert dev.info()["n_reads"] == len(offs) - 1, what
    if not np.array_equal(out["offsets"], offs):
        r = int(np.flatnonzero(out["offsets"] != offs)[0]) - 1
        raise AssertionError(f"{what}: read {r} has {int(out['offsets'][r + 1] - out['offsets'][r])} minimizers, expected {int(offs[r + 1] - offs[r])}")
    if not np.array_equal(out["minimizers"], mins):
        at = int(np.flatnonzero(out["minimizers"] != mins)[0])
        r = int(np.searchsorted(offs, at, side="right")) - 1
        raise AssertionError(f"{what}: read {r} differs at its minimizer {at - int(offs[r])}")


def _purge_and_check(ctx, orc, lists, first_k, last_k, what, idempotent=False):
    """One purge call over `lists` as one CSR batch against the oracle; returns the oracle's lists."""
    exp = [orc.purge_palindrome(x, first_k, last_k) for x in lists]
    emins, eoffs = _csr(exp)
    dev = ctx.purge_palindromes(ctx.minimizers_from_host(*_csr(lists)), first_k, last_k)
    _assert_same(dev, emins, eoffs, what)
    if idempotent:
        _assert_same(ctx.purge_palindromes(dev, first_k, last_k), emins, eoffs, f"{what}, purged twice")
    return exp


def _lost(lists, exp):
    return np.array([len(a) - len(b) for a, b in zip(lists, exp)])


# ---- 1. dense lists on both sides of the LDS border ------------------------------------------------------------------------------
PAIRS = [(2, 3), (2, 100), (3, 4), (3, 9), (4, 5), (4, 6), (4, 100), (5, 100), (6, 8), (7, 200), (4, 4), (5, 3)]
DENSE_LENGTHS = list(range(0, 13)) + [15, 16, 17, 18, 31, 32, 33, 34, 94, 95, 96, 97, 98, 99, 130, 200, 400]
_dense = None


def _dense_lists():
    """(lists, alphabet of each; 0 = a clean list of distinct values): three seeded random lists per (alphabet, length), a clean
    list after every eleventh."""
    global _dense
    if _dense is None:
        rng = np.random.default_rng(20261018)
        lists, alpha = [], []
        for a in (2, 3, 4, 12):
            for n in DENSE_LENGTHS:
                for _ in range(3):
                    lists.append(rng.integers(0, a, n).astype(np.uint32)); alpha.append(a)
                    if len(lists) % 12 == 11:
                        lists.append((1000 + rng.permutation(500)[: int(rng.integers(0, 150))]).astype(np.uint32)); alpha.append(0)
        _dense = (lists, np.array(alpha))
    return _dense


@pytest.mark.parametrize("first_k,last_k", PAIRS)
def test_dense_lists_both_sides_of_the_lds_border(ctx, orc, first_k, last_k):
    lists, alpha = _dense_lists()
    lens = np.array([len(x) for x in lists])
    assert (alpha == 0).sum() >= 20 and set(lens[alpha > 0].tolist()) == set(DENSE_LENGTHS)
    exp = _purge_and_check(ctx, orc, lists, first_k, last_k, f"dense lists at ({first_k}, {last_k})", idempotent=True)
    lost = _lost(lists, exp)
    assert not lost[alpha == 0].any()                      # distinct values: nothing to drop
    if last_k <= first_k:                                  # no k to look at: (4,4), (5,3)
        assert not lost.any()
        return
    # both replay paths drop at every pair (first_k = 2, odd first_k, last_k = first_k + 1 among them) ...
    assert lost[(lens <= LDS_MAX) & (lens >= 15)].astype(bool).sum() >= 20 and lost[lens > LDS_MAX].astype(bool).sum() >= 10
    # ... and on both sides next to the border
    assert lost[lens == LDS_MAX].any() and lost[lens == LDS_MAX + 1].any()
    if (first_k, last_k) == (4, 100):
        small = (alpha > 0) & (alpha <= 4) & (lens >= 8)
        assert 2 * lost[small].astype(bool).sum() >= small.sum()
        for n in sorted(set(lens[(alpha > 0) & (lens > LDS_MAX)].tolist())):
            assert lost[(alpha > 0) & (lens == n)].max() >= 10, n


# ---- 2. suspects that are not palindromes, and where the centre sits -----------------------------------------------------------
def _distinct(rng, n):
    """n distinct values in a random order (n * 7919 + 2^30 stays below 2^32)."""
    return (int(rng.integers(1 << 20, 1 << 30)) + 7919 * rng.permutation(n)).astype(np.uint32)


def test_clean_suspects_among_palindromic_and_clean_reads(ctx, orc):
    """With first_k = 4 an `a a` pair or an `a b a` triple in otherwise distinct values is what the detector lists and the replay
    must leave alone; between clean reads and really palindromic ones, whose drops move every later read's offset."""
    rng = np.random.default_rng(77)
    lists, kind = [], []
    for n in (2, 3, 4, 5, 15, 16, 17, 18, 32, 33, 95, 96, 97, 98, 130, 200):
        for at in sorted({0, 1, n // 2, n - 3, n - 2}):
            for width in (2, 3):                           # a a / a b a
                if at < 0 or at + width > n:
                    continue
                x = _distinct(rng, n); x[at + width - 1] = x[at]
                lists.append(x); kind.append("suspect")
        lists.append(_distinct(rng, n)); kind.append("clean")
        y = _distinct(rng, max(n, 4)); s = int(rng.integers(0, len(y) - 3)); y[s + 3] = y[s]; y[s + 2] = y[s + 1]
        lists.append(y); kind.append("palindromic")
        lists.append(rng.integers(0, 3, n).astype(np.uint32)); kind.append("dense")
    order = rng.permutation(len(lists))
    lists = [lists[i] for i in order]; kind = np.array(kind)[order]
    exp = _purge_and_check(ctx, orc, lists, 4, 100, "clean suspects")
    lost = _lost(lists, exp)
    assert (kind == "suspect").sum() >= 100 and not lost[kind == "suspect"].any() and not lost[kind == "clean"].any()
    assert (lost[kind == "palindromic"] == 1).all() and lost[kind == "dense"].sum() > 200
    # unchanged reads behind dropped minimizers: their offsets shift
    before = np.concatenate([[0], np.cumsum(lost)[:-1]])
    assert ((kind == "suspect") & (before > 0)).sum() >= 90 and ((kind == "clean") & (before > 0)).sum() >= 10
    lens = np.array([len(x) for x in lists])
    assert ((kind == "suspect") & (lens > LDS_MAX)).sum() >= 20       # clean suspects on the global-memory path too


def test_batch_of_suspects_none_of_which_is_palindromic(ctx, orc):
    """Every listed read comes back from the replay as it went in: the output is the input, through `work` and the gather."""
    rng = np.random.default_rng(78)
    lists = []
    for n in (2, 3, 7, 40, 96, 97, 300):
        for width in (2, 3):
            if width <= n:
                x = _distinct(rng, n); at = int(rng.integers(0, n - width + 1)); x[at + width - 1] = x[at]
                lists.append(x)
        lists.append(_distinct(rng, n))
    exp = _purge_and_check(ctx, orc, lists, 4, 100, "suspects, none palindromic")
    assert not _lost(lists, exp).any()


def test_no_suspect_at_all_is_a_copy(ctx, orc):
    """No read has two equal minimizers one or two apart: mdbg_purge_palindromes copies the CSR input."""
    rng = np.random.default_rng(79)
    lists = [_distinct(rng, int(n)) for n in [0, 1, 2, 3, 0, 96, 97, 500] + list(rng.integers(0, 60, 300))]
    for x in lists:
        assert len(x) < 2 or ((x[1:] != x[:-1]).all() and (x[2:] != x[:-2]).all())
    mins, offs = _csr(lists)
    for first_k, last_k in ((4, 100), (2, 100)):
        exp = _purge_and_check(ctx, orc, lists, first_k, last_k, f"no suspect at ({first_k}, {last_k})")
        assert not _lost(lists, exp).any()
        _assert_same(ctx.purge_palindromes(ctx.minimizers_from_host(mins, offs), first_k, last_k), mins, offs, "copy of the input")


CENTRE_N = (4, 5, 16, 17, 18, 33, 96, 97)


@pytest.mark.parametrize("pattern,first_k", [("aa", 2), ("aba", 2), ("aba", 3), ("abba", 3), ("abba", 4), ("abcba", 4), ("abcba", 5), ("abccba", 5)])
def test_one_planted_palindrome_at_every_start(ctx, orc, pattern, first_k):
    """One palindrome, at every start s = 0 .. n - len in a list of otherwise distinct values, one list per s: the centre sweeps the
    read's first and last elements, the detector's 16-lane stride (i = sub; i += 16, the i + 2 < n guard), and both replay paths.
    The smallest window the reference finds is the pattern itself (length first_k, or first_k + 1 where the pattern's parity is
    the other one); its first element goes, and nothing else."""
    rng = np.random.default_rng(1000 + 10 * len(pattern) + first_k)
    w = len(pattern)
    lists, start = [], []
    for n in CENTRE_N:
        for s in range(0, n - w + 1):
            x = _distinct(rng, n)
            for j in range(w // 2):
                x[s + w - 1 - j] = x[s + j]
            lists.append(x); start.append(s)
    assert len(lists) >= 240
    exp = _purge_and_check(ctx, orc, lists, first_k, 100, f"{pattern} planted, first_k = {first_k}")
    for x, e, s in zip(lists, exp, start):
        assert e.tolist() == np.delete(x, s).tolist(), (len(x), s)


# ---- 3. more reads than one pass of the grids ------------------------------------------------------------------------------------
def test_more_reads_than_two_passes_of_the_grids(ctx, orc):
    """purge_detect_kernel runs n_cu * 16 blocks of 16 reads, gather_prefix_kernel n_cu * 32: with more than 2 * n_cu * 32 * 16 reads
    both go round their grid-stride loops more than twice, and the fix kernel gets more than a hundred thousand suspects.  A pool
    of 3,000 short lists, tiled in a seeded order; the oracle runs over the pool.  first_k = 3: `a b a` and `a b b a` both count."""
    n_cu = ctx.device_info()["n_cu"]
    n_reads = 2 * n_cu * 32 * 16 + n_cu * 32 * 4 + 77
    rng = np.random.default_rng(303)
    pool = [rng.integers(0, 6, int(n)).astype(np.uint32) for n in rng.integers(0, 13, 3000)]
    exp = [orc.purge_palindrome(x, 3, 100) for x in pool]
    assert 3 * _lost(pool, exp).astype(bool).sum() >= len(pool)
    idx = rng.permutation(np.arange(n_reads) % len(pool))
    assert n_reads > 2 * n_cu * 32 * 16 and _lost(pool, exp).astype(bool)[idx].sum() > 100_000

    def tiled(lists):
        flat, off = _csr(lists)
        off = off.astype(np.int64)
        lens = (off[1:] - off[:-1])[idx]
        offs = np.concatenate([[0], np.cumsum(lens)])
        src = np.repeat(off[:-1][idx] - offs[:-1], lens) + np.arange(offs[-1])
        return flat[src], offs.astype(np.uint64)

    mins, offs = tiled(pool)
    emins, eoffs = tiled(exp)
    for r in (0, 1, n_reads // 2, n_reads - 1):            # the tiling itself
        assert mins[int(offs[r]): int(offs[r + 1])].tolist() == pool[idx[r]].tolist()
        assert emins[int(eoffs[r]): int(eoffs[r + 1])].tolist() == exp[idx[r]].tolist()
    _assert_same(ctx.purge_palindromes(ctx.minimizers_from_host(mins, offs), 3, 100), emins, eoffs, f"{n_reads} tiled reads")


# ---- 4. long reads -----------------------------------------------------------------------------------------------------------------
def test_long_reads_among_short(ctx, orc):
    """A read of more than 2^16 distinct minimizers with `a b b a` at its very start, in its middle and as its last four elements,
    one of 20,000 with an `a b c b a`, one of exactly 97 with a palindrome at its end, among ordinary short lists: the
    global-memory replay with indices beyond 16 bits, and the shift after a drop over the whole read.  (4, 12) keeps the
    brute-force oracle at about a second."""
    rng = np.random.default_rng(404)
    lists = [rng.integers(0, 6, int(n)).astype(np.uint32) for n in rng.integers(0, 40, 120)]
    lists += [_distinct(rng, int(n)) for n in rng.integers(0, 200, 40)]
    lists = [lists[i] for i in rng.permutation(len(lists))]
    big = (5_000_000 + rng.permutation(66_000)).astype(np.uint32)
    for s in (0, 33_001, 66_000 - 4):
        big[s + 3] = big[s]; big[s + 2] = big[s + 1]
    mid = (6_000_000 + rng.permutation(20_000)).astype(np.uint32)
    mid[12_345 + 4] = mid[12_345]; mid[12_345 + 3] = mid[12_345 + 1]
    edge = (7_000_000 + rng.permutation(97)).astype(np.uint32)
    edge[96] = edge[93]; edge[95] = edge[94]
    at = {50: big, 51: mid, 100: edge}
    for i in sorted(at):
        lists.insert(i, at[i])
    exp = _purge_and_check(ctx, orc, lists, 4, 12, "long reads among short", idempotent=True)
    lost = _lost(lists, exp)
    assert len(lists[50]) == 66_000 > 1 << 16 and len(lists[51]) == 20_000 and len(lists[100]) == 97
    assert (lost[50], lost[51], lost[100]) == (3, 1, 1)
    assert exp[50].tolist() == np.delete(big, [0, 33_001, 66_000 - 4]).tolist()
    assert lost[:50].sum() > 0 and lost[101:].sum() > 0


# ---- 5. scattered input that really contains palindromes -----------------------------------------------------------------------
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def _hairpin_batch(density, hpc):
    """Random reads, and hairpins X . revcomp(X) -- their own reverse complement, so their canonical minimizer list is a palindrome --
    one, two and three copies long, sized for about 40 .. 350 minimizers at this density."""
    rng = np.random.default_rng(505 + int(hpc) + int(density * 1000))
    per_base = density * (0.75 if hpc else 1.0)            # random DNA keeps three bases of four under homopolymer compression

    def rnd(n):
        return bytes(synth.CODE2ASCII[rng.integers(0, 4, int(n))])

    seqs = [rnd(n) for n in rng.integers(300, 4000, 150)]
    hairpins = []
    for copies, targets in ((1, (40, 60, 75, 85, 110, 120, 150, 220, 300)), (2, (120, 250, 320)), (3, (150, 300))):
        for t in targets:
            x = rnd(t / per_base / (2 * copies))
            hairpins.append((x + x.translate(_RC)[::-1]) * copies)
    where = dict(zip(rng.choice(len(seqs), len(hairpins), replace=False).tolist(), hairpins))
    out, is_hairpin = [], []
    for i, s in enumerate(seqs):
        if i in where:
            out.append(where[i]); is_hairpin.append(True)
        out.append(s); is_hairpin.append(False)
    return out, np.array(is_hairpin)


@pytest.mark.parametrize("hpc", [True, False])
@pytest.mark.parametrize("density", [0.02, 0.05])
def test_scattered_scan_output_with_hairpin_reads(ctx, orc, density, hpc):
    """The purge reads a fresh scan output where the block kernel left it (mdbg_minimizers::scattered: begin[r], cnt[r], slack in
    between) -- here with reads that lose minimizers on both replay paths -- and the same reads in CSR order must give the same."""
    seqs, is_hairpin = _hairpin_batch(density, hpc)
    lists = [orc.read_selection(s, None, K=15, density=density, hpc=hpc)["minimizers"] for s in seqs]
    exp = [orc.purge_palindrome(x, 4, 100) for x in lists]
    lens, lost = np.array([len(x) for x in lists]), _lost(lists, exp)
    assert is_hairpin.sum() == 14 and (lost[is_hairpin] >= 1).all() and lost[is_hairpin].max() >= 3
    for x, hp in zip(lists, is_hairpin):
        assert not hp or np.array_equal(x, x[::-1])
    assert (is_hairpin & (lens <= LDS_MAX)).sum() >= 3 and (is_hairpin & (lens > LDS_MAX)).sum() >= 3 and lens.max() < 400
    mins, offs = _csr(lists)
    emins, eoffs = _csr(exp)
    reads = ctx.reads_from_ascii(seqs)
    # scattered: nothing touches the scan output between the scan and the purge
    fresh = ctx.scan(reads, K=15, density=density, hpc=hpc)
    purged = ctx.purge_palindromes(fresh, 4, 100)
    _assert_same(purged, emins, eoffs, "purge of the fresh scan output")
    _assert_same(ctx.purge_palindromes(purged, 4, 100), emins, eoffs, "purge of the fresh scan output, purged twice")
    # ... and it was in the scattered form: bringing it into CSR order is one launch of the compaction kernel, now
    ctx.timing(True); ctx.timing_reset()
    try:
        h = fresh.to_host(full=False)
        assert ctx.timing_get("scan_compact")[1] == 1
    finally:
        ctx.timing(False)
    assert np.array_equal(h["minimizers"], mins) and np.array_equal(h["offsets"], offs)
    # CSR: a second scan of the same reads, read back first
    second = ctx.scan(reads, K=15, density=density, hpc=hpc)
    h = second.to_host(full=False)
    assert np.array_equal(h["minimizers"], mins) and np.array_equal(h["offsets"], offs)
    _assert_same(ctx.purge_palindromes(second, 4, 100), emins, eoffs, "purge of the scan output in CSR order")


# ---- 7. the reference's own outputs at the new corners -----------------------------------------------------------------------------
def test_purge_long_lists_golden(ctx):
    """fn/purge_long.json: Commons::purgePalindrome itself (refdrv fn_purge) on lists of 90 .. 400 minimizers."""
    with open(os.path.join(H.GOLDEN, "fn", "purge_long.json")) as f:
        g = json.load(f)["purge_long"]
    lists = [np.array(line.split(), dtype=np.uint32) for line in g["inputs"]]
    mins, offs = _csr(lists)
    assert len(g["outputs"]) == 5
    for key, outs in g["outputs"].items():
        first_k, last_k = map(int, key.split("_"))
        exp = [np.array(line.split(), dtype=np.uint32) for line in outs]
        assert len(exp) == len(lists) and _lost(lists, exp).sum() > 500
        _assert_same(ctx.purge_palindromes(ctx.minimizers_from_host(mins, offs), first_k, last_k), *_csr(exp), f"purge_long at {key}")
