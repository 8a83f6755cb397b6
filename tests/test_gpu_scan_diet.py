"""What the block kernel (scan.hip, scan_fast_kernel) does outside its hash: the block's set-up (table image and ring cleared with
16-byte stores, a wave's second read starting on the ring the first one left), the 2-mer complexity bound in its +-1 form
(csrc/complexity_dev.hpp) with its one compare per read, and the 32-bit wave sum behind that compare.  Minimizers, positions,
directions and read flags against the oracle.  Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

from metamdbg_amd import synth

pytestmark = pytest.mark.gpu


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


def _ascii(codes) -> bytes:
    return bytes(synth.CODE2ASCII[np.asarray(codes, dtype=np.int64)])


def _no_runs(rng, n):
    """n codes, no two neighbours equal: the compressed length is n whatever is stretched afterwards."""
    return np.cumsum(np.concatenate([rng.integers(0, 4, 1), rng.integers(1, 4, n - 1)])) % 4 if n > 1 else rng.integers(0, 4, n)


def _with_compressed_length(rng, n, hpc):
    c = _no_runs(rng, n)
    return _ascii(np.repeat(c, rng.choice([1, 1, 2, 3], len(c))) if hpc else c)


def _compare(ctx, orc, seqs, K, density, hpc):
    """Scan with the read filters on; every read's values, positions, directions and flags against readSelection's."""
    reads = ctx.reads_from_ascii(seqs)
    m = ctx.scan(reads, K=K, density=density, hpc=hpc, apply_read_filters=True)
    h = m.to_host()
    assert len(h["offsets"]) == len(seqs) + 1
    low = []
    for i, s in enumerate(seqs):
        e = orc.read_selection(s, None, K=K, density=density, hpc=hpc)
        a, b = int(h["offsets"][i]), int(h["offsets"][i + 1])
        where = (K, density, hpc, i, len(s))
        assert int(h["flags"][i]) == (1 if e["low_complexity"] else 0), where          # MDBG_READ_LOW_COMPLEXITY, and no internal bit left
        assert b - a == len(e["minimizers"]), where
        assert np.array_equal(h["minimizers"][a:b], e["minimizers"]) and np.array_equal(h["pos"][a:b], e["pos"]) \
            and np.array_equal(h["dir"][a:b], e["dir"]), where
        low.append(bool(e["low_complexity"]))
    m.free()
    reads.free()
    return np.array(low)


# ---- (a) set-up and the second read of a wave ------------------------------------------------------------------------------------
# A wave takes read w and then read w + (number of waves) = w + 4 ceil(n / 8): with 1 read one wave works and three idle, with 7 the
# block's fourth wave has no second read, with 8 every wave has two, with 9 a second block is nearly empty, 37 leaves a part block.
def _setup_batch(n, K, hpc):
    rng = np.random.default_rng(500 + 8 * n + K + int(hpc))
    long_read = _ascii(np.repeat(rng.integers(0, 4, 34000), rng.choice([1, 1, 2], 34000))[:40000]) if hpc else _ascii(rng.integers(0, 4, 40000))
    assert len(long_read) == 40000                                              # laps the ring of 16 384 bases, compressed or not
    specials = [_ascii(rng.integers(0, 4, 1))] + [_with_compressed_length(rng, 2048 + K + d, hpc) for d in (-1, 0, 1)]
    short = _ascii(rng.integers(0, 4, K - 2))
    if n == 1:
        return [long_read]
    others = specials + [_ascii(rng.integers(0, 4, int(rng.integers(1, 9000)))) for _ in range(n)]
    seqs = [long_read] + others[: n - 2]
    seqs.insert(4 * ((n + 7) // 8), short)                                      # the read wave 0 takes after the 40 kb one
    return seqs


@pytest.mark.parametrize("K", [15, 13])
@pytest.mark.parametrize("hpc", [True, False])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 37])
def test_setup_and_second_read_of_a_wave(ctx, orc, n, hpc, K):
    seqs = _setup_batch(n, K, hpc)
    assert len(seqs) == n
    if n >= 7:
        second = 4 * ((n + 7) // 8)
        assert len(seqs[0]) == 40000 and len(seqs[second]) < K
        assert sum(len(s) == 1 for s in seqs) >= 1
        if hpc:
            got = {orc.read_selection(s, None, K=K, density=0.005, hpc=True)["hpc_length"] for s in seqs}
            assert {2048 + K - 1, 2048 + K, 2048 + K + 1} <= got
    ctx.timing(True); ctx.timing_reset()
    try:
        _compare(ctx, orc, seqs, K, 0.005, hpc)
        assert ctx.timing_get("scan")[1] == 1                                   # the block kernel alone: no read was handed on
    finally:
        ctx.timing(False)


# ---- (b) the bound ---------------------------------------------------------------------------------------------------------------
BOUND_LENGTHS = [65, 66, 67, 97, 98, 2048, 2049, 4097, 10000]
BOUND_SEED = 7


def _gc30(rng, n):
    return rng.choice(4, n, p=[0.35, 0.15, 0.35, 0.15])                         # codes A C T G


def _bound_batch(seed):
    rng = np.random.default_rng(seed)
    units = [[0], [0, 1], [0, 0, 1], [0, 1, 3, 2]]                              # A, AC, AAC, ACGT
    seqs = []
    for n in BOUND_LENGTHS:
        for kind in range(7):
            for rep in range(4):
                if kind == 0: c = rng.integers(0, 4, n)
                elif kind == 1: c = _gc30(rng, n)
                elif kind <= 5: c = np.resize(np.roll(units[kind - 2], rep), n)
                else:           # random with a low-complexity third (more or less), the unit and the two letters of the rest by chance
                    c = rng.integers(0, 4, n)
                    k = int(n * rng.uniform(0.25, 0.45)); at = int(rng.integers(0, n - k + 1))
                    c[at: at + k] = np.resize(units[int(rng.integers(0, 4))], k) if rep < 3 else rng.choice([0, 2], k)
                seqs.append(_ascii(c))
    for n in (2048, 4097, 10000):                                               # two letters at random: many equal 2-mers, 3-mers within the limit
        seqs.append(_ascii(rng.choice([0, 2], n)))
        seqs.append(_ascii(rng.choice([1, 3], n)))
    return seqs


def _bound_says_suspect(s: bytes) -> bool:
    """The kernels' bound, counted directly: sum over the words 0 .. nW of weight x (sum of squared 2-mer counts of the word's 32
    positions) > 332 nW (complexity_dev.hpp; the +-1 form the device runs is checked against this count by
    tests/host/test_complexity_bound.cpp)."""
    L = len(s)
    if L < 66:
        return False
    nW = (L - 66) // 32 + 1
    c = (np.frombuffer(s, np.uint8) >> 1) & 3
    pairs = (c[:-1].astype(np.int64) * 4 + c[1:])[: 32 * (nW + 1)]
    counts = np.bincount(np.arange(len(pairs)) // 32 * 16 + pairs, minlength=16 * (nW + 1)).reshape(nW + 1, 16)
    sq = (counts.astype(np.int64) ** 2).sum(axis=1)
    weight = np.full(nW + 1, 2); weight[0] = 1; weight[nW] = 1
    return int((weight * sq).sum()) > 332 * nW


@pytest.mark.parametrize("hpc", [True, False])
def test_complexity_bound_and_exact_pass(ctx, orc, hpc):
    seqs = _bound_batch(BOUND_SEED)
    assert 250 <= len(seqs) <= 262
    suspect = np.array([_bound_says_suspect(s) for s in seqs])
    ctx.timing(True); ctx.timing_reset()
    try:
        low = _compare(ctx, orc, seqs, 15, 0.005, hpc)
        exact_launches = ctx.timing_get("complexity_exact")[1]
    finally:
        ctx.timing(False)
    assert not (low & ~suspect).any()                      # the bound is one: no dropped read passes it
    # all three outcomes, or the comparison above proves nothing: dropped, suspect but kept by the exact pass, clean
    assert low.sum() >= 20 and (suspect & ~low).sum() >= 10 and (~suspect).sum() >= 20, (low.sum(), (suspect & ~low).sum(), (~suspect).sum())
    assert exact_launches == 1


# ---- the wave sum behind the compare ---------------------------------------------------------------------------------------------
def test_complexity_sum_at_the_32_bit_limit_and_beyond(ctx, orc):
    """Below 2^24 bases a lane adds its words up in 32 bits and the wave's sum is taken in 32 bits: poly-A of 2^24 - 1 bases is the
    largest sum that way takes (2 nW x 3840 = 4 026 462 720 of 4 294 967 296).  From 2^24 bases on the tiles fold into a 64-bit total:
    a clean read, a suspect the exact pass keeps and one it drops, at a density that leaves them in the block kernel's stage."""
    rng = np.random.default_rng(11)
    n = (1 << 24) + 77
    runs = np.repeat(_no_runs(rng, n // 1000 + 1), 1000)[:n]
    seqs = [_ascii(np.zeros((1 << 24) - 1, np.int64)), _ascii(rng.integers(0, 4, n)), _ascii(rng.choice([0, 2], n)), _ascii(runs),
            _ascii(rng.integers(0, 4, 5000))]
    ctx.timing(True); ctx.timing_reset()
    try:
        low = _compare(ctx, orc, seqs, 15, 1e-5, True)
        assert ctx.timing_get("scan")[1] == 1 and ctx.timing_get("complexity_exact")[1] == 1
    finally:
        ctx.timing(False)
    assert low.tolist() == [True, False, False, True, False]
