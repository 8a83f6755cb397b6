"""The pre-filtered variant of the block kernel (scan.hip, scan_fast_kernel<.., PFW>; csrc/prefilter.hpp): a bitmap of the selected keys
in LDS instead of the candidate hash, the positions that pass confirmed with the full hash before they are emitted, 16 waves a workgroup
that deal the workgroup's reads out among themselves.  Every case against the oracle read by read -- values, positions, directions,
flags, counts -- with the library's own counters (mdbg_scan_info) showing which kernel ran, and with the oracle's answer showing that
the case selects minimizers where it says so.  Each case also runs with "scan_prefilter_log2_bits" = 10: a bitmap of 1024 bits, all
set, so that every position reaches the confirmation and its list overflows.  Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

from metamdbg_amd import synth

pytestmark = pytest.mark.gpu

K = 15
DENSITY = 0.005
BLOCK = 2048                     # positions of a block
STAGE = 176                      # rows a wave of the variant stages for one read (PF_STAGE_CAP)


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module", params=[0, 10], ids=["bitmap19", "bitmap10"])
def ctx(request):
    from metamdbg_amd import capi
    c = capi.Context(0)
    c.set_option("scan_prefilter", 1)
    c.set_option("scan_prefilter_log2_bits", request.param)
    c.log2_bits = request.param
    yield c
    c.close()


def _ascii(codes) -> bytes:
    return bytes(synth.CODE2ASCII[np.asarray(codes, dtype=np.int64)])


def _no_runs(rng, n):
    """n codes, no two neighbours equal: the compressed length is n whatever is stretched afterwards."""
    return np.cumsum(np.concatenate([rng.integers(0, 4, 1), rng.integers(1, 4, n - 1)])) % 4 if n > 1 else rng.integers(0, 4, n)


def _compressed(rng, n) -> bytes:
    """A read whose homopolymer-compressed length is n."""
    c = _no_runs(rng, n)
    return _ascii(np.repeat(c, rng.choice([1, 1, 2, 3], len(c))))


_EXPECTED = {}


def _expected(orc, s, k, density, hpc):
    """The oracle's record of a read, computed once per (read, parameters)."""
    key = (s, k, density, hpc)
    if key not in _EXPECTED:
        _EXPECTED[key] = orc.read_selection(s, None, K=k, density=density, hpc=hpc)
    return _EXPECTED[key]


def _compare(ctx, orc, seqs, k=K, density=DENSITY, hpc=True, prefiltered=True):
    """Scan; every read against readSelection's record; which kernel ran.  Returns the oracle's records."""
    before = ctx.scan_info()
    reads = ctx.reads_from_ascii(seqs)
    m = ctx.scan(reads, K=k, density=density, hpc=hpc, apply_read_filters=True)
    h = m.to_host()
    m.free()
    reads.free()
    after = ctx.scan_info()
    if prefiltered:      # "split": the reads too long for the variant's stage in a launch of the four-wave kernel behind it
        assert after["prefiltered_launches"] == before["prefiltered_launches"] + 1, (before, after)
        assert after["block_launches"] == before["block_launches"] + (1 if prefiltered == "split" else 0), (before, after)
        assert after["bitmap_log2_bits"] == (ctx.log2_bits or 19)
    else:
        assert after["prefiltered_launches"] == before["prefiltered_launches"] and after["block_launches"] == before["block_launches"] + 1, (before, after)
    assert len(h["offsets"]) == len(seqs) + 1
    exp = []
    for i, s in enumerate(seqs):
        e = _expected(orc, s, k, density, hpc)
        a, b = int(h["offsets"][i]), int(h["offsets"][i + 1])
        where = (k, density, hpc, i, len(s), e["hpc_length"])
        assert int(h["flags"][i]) == (1 if e["low_complexity"] else 0), where
        assert b - a == len(e["minimizers"]), where
        assert np.array_equal(h["minimizers"][a:b], e["minimizers"]) and np.array_equal(h["pos"][a:b], e["pos"]) \
            and np.array_equal(h["dir"][a:b], e["dir"]), where
        exp.append(e)
    return exp


def _mixed(rng, n):
    """n reads from shorter than l to about three blocks, compressed."""
    lengths = [K - 3, K, K + 1, 3 * BLOCK + 500, 40, BLOCK + K, 700, 2 * BLOCK + 90]
    return [_compressed(rng, lengths[i % len(lengths)] if i < len(lengths) else int(rng.integers(1, 3 * BLOCK))) for i in range(n)]


# ---- batch sizes around one workgroup's chunk of 16 x scan_reads_per_wave reads ---------------------------------------------------
@pytest.mark.parametrize("n,per_wave", [(1, 2), (15, 1), (16, 1), (17, 1), (33, 1), (33, 2)])
def test_batch_sizes_around_a_workgroups_chunk(ctx, orc, n, per_wave):
    seqs = _mixed(np.random.default_rng(100 + n), n)
    if n == 1:
        seqs = [_compressed(np.random.default_rng(101), 3 * BLOCK + 500)]
    ctx.set_option("scan_reads_per_wave", per_wave)
    try:
        exp = _compare(ctx, orc, seqs)
    finally:
        ctx.set_option("scan_reads_per_wave", 2)
    assert sum(len(e["minimizers"]) for e in exp) >= 5 * ((n + 7) // 8)            # the long reads select


# ---- compressed lengths around the block and the tail -------------------------------------------------------------------------------
def test_compressed_lengths_at_the_block_and_tail_boundaries(ctx, orc):
    rng = np.random.default_rng(7)
    # a read of compressed length c has c - l positions that are followed by a base
    npos = [0, 1, BLOCK - 1, BLOCK, BLOCK + 1] + [2 * BLOCK + t for t in (1, 63, 64, 65, BLOCK - 1)]
    seqs = [_compressed(rng, p + K) for p in npos] + [_compressed(rng, c) for c in (BLOCK - 1 + K - 1, BLOCK + K - 1, BLOCK + 1 + K - 1)]
    exp = _compare(ctx, orc, seqs)
    assert [e["hpc_length"] for e in exp[:len(npos)]] == [p + K for p in npos]
    assert all(len(e["minimizers"]) >= 1 for e in exp[2:]) and all(len(e["minimizers"]) == 0 for e in exp[:2])


# ---- planted reads: concatenated selected windows ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def selected_windows(orc):
    """Compressed 15-mers the oracle selects, as they stood in a random run-free sequence (codes, reading order)."""
    rng = np.random.default_rng(2026)
    c = _no_runs(rng, 300_000)
    _, pos, _ = orc.minimizer_parse(_ascii(c), K, DENSITY, True)
    assert len(pos) >= 1000
    return [c[p: p + K] for p in pos]


def _planted(windows, n, start):
    """n of the windows end to end, each starting with another base than its predecessor ends with."""
    out, last, i = [], -1, start
    while len(out) < n:
        w = windows[i % len(windows)]
        i += 1
        if int(w[0]) != last:
            out.append(w)
            last = int(w[-1])
    return np.concatenate(out)


def test_reads_planted_with_selected_windows(ctx, orc, selected_windows):
    """Every 15th position selected: a lane's span of 32 holds two or three true minimizers, a block 136 -- a read of 150 windows
    fills most of the stage, one of 250 outgrows it where the four-wave kernel's stage of 384 rows would have held it, reads of 400
    and 1000 outgrow both (once and several times over); all three go the way of every read that outgrows a stage."""
    rng = np.random.default_rng(5)
    plain = [_compressed(rng, 1200) for _ in range(3)]
    planted = [_ascii(_planted(selected_windows, n, 37 * n)) for n in (11, 150, 400, 1000, 250)]
    seqs = [plain[0], planted[1], planted[0], plain[1], planted[2], planted[3], plain[2], planted[4]]
    exp = _compare(ctx, orc, seqs)
    for i, n in ((2, 11), (1, 150), (4, 400), (5, 1000), (7, 250)):
        # (the first window is the read's trimmed first position, the last has no base behind it; a window across a joint is selected by chance)
        assert exp[i]["hpc_length"] == K * n and n - 2 <= len(exp[i]["minimizers"]) <= n + n // 5 + 8, (n, len(exp[i]["minimizers"]))
    assert len(exp[1]["minimizers"]) <= STAGE < len(exp[4]["minimizers"]) and len(exp[5]["minimizers"]) > 5 * STAGE
    assert STAGE < len(exp[7]["minimizers"]) <= 384


# ---- reads too long for the variant's stage: the four-wave kernel's, in the same call ---------------------------------------------
LEN_LIMIT = int((STAGE - 24) / (DENSITY * 0.8 * 1.4))           # 27 142 bases: mdbg_scan's pf_len_limit


@pytest.mark.parametrize("n_long,split", [(1, True), (6, False)])
def test_long_reads_beside_short_ones(ctx, orc, n_long, split):
    """A batch whose average read fits the variant's stage and some do not.  Holding at most 1/32 of the bases, the long reads are
    scanned by a launch of the four-wave kernel and the rest by the variant -- every read the oracle's, also those just below and
    at the limit; holding more, they keep the whole batch on the four-wave kernel."""
    rng = np.random.default_rng(29 + n_long)
    short = [_compressed(rng, int(rng.integers(200, 2 * BLOCK))) for _ in range(1200)]
    long_ = [_compressed(rng, 9 * BLOCK + 77 * i) for i in range(n_long)]
    edge = [_ascii(_no_runs(rng, LEN_LIMIT - 1)), _ascii(_no_runs(rng, LEN_LIMIT)), _ascii(_no_runs(rng, LEN_LIMIT + 1))]
    seqs = short[:7] + long_[:1] + short[7:20] + edge + long_[1:] + short[20:]
    total, over = sum(len(s) for s in seqs), sum(len(s) for s in seqs if len(s) >= LEN_LIMIT)
    assert all(len(s) > LEN_LIMIT + 2000 for s in long_) and total / len(seqs) < LEN_LIMIT / 2
    assert (over * 32 <= total) == split and abs(over * 32 - total) > total // 4              # well on either side of the rule
    exp = _compare(ctx, orc, seqs, prefiltered="split" if split else False)
    assert all(len(_expected(orc, s, K, DENSITY, True)["minimizers"]) >= 60 for s in long_ + edge)
    assert sum(len(e["minimizers"]) for e in exp) >= 300


# ---- more than three blocks: deferral and the release of the ring ---------------------------------------------------------------
def test_reads_of_many_blocks(ctx, orc):
    rng = np.random.default_rng(9)
    seqs = [_compressed(rng, 5 * BLOCK + 300), _compressed(rng, 7 * BLOCK + 1), _compressed(rng, 30)]      # (25 kb: the longest the variant takes)
    exp = _compare(ctx, orc, seqs)
    assert len(exp[0]["minimizers"]) >= 30 and len(exp[1]["minimizers"]) >= 40


# ---- the bitmap's cache: key and lifetime ---------------------------------------------------------------------------------------
def test_two_densities_in_turn_and_two_contexts_together(ctx, orc):
    from metamdbg_amd import capi
    rng = np.random.default_rng(13)
    seqs = [_compressed(rng, int(rng.integers(500, 2 * BLOCK + 600))) for _ in range(20)]
    other = capi.Context(0)
    try:
        other.set_option("scan_prefilter", 1)
        other.set_option("scan_prefilter_log2_bits", ctx.log2_bits)
        other.log2_bits = ctx.log2_bits
        _compare(ctx, orc, seqs, density=0.003)                           # whatever ran before: the context's bitmap is another density's now
        built = ctx.scan_info()["bitmaps_built"]
        counts = []
        for density in (0.005, 0.002, 0.002, 0.005):
            exp = _compare(ctx, orc, seqs, density=density)
            _compare(other, orc, seqs, density=0.003)                   # another context, another key, alive beside it
            counts.append(sum(len(e["minimizers"]) for e in exp))
        assert ctx.scan_info()["bitmaps_built"] == built + 3             # rebuilt when the density changes, kept when it does not
        assert other.scan_info()["bitmaps_built"] == 1
        assert counts[0] == counts[3] > counts[1] == counts[2] > 20
        if not ctx.log2_bits:
            assert ctx.scan_info()["bitmap_bits_set"] == 45657            # density 0.005f: tests/host/test_prefilter_bitmap.cpp
    finally:
        other.close()


@pytest.mark.parametrize("reserve,waves", [(28672, 16), (60000, 8), (100000, 0)])
def test_lds_reserve_is_honoured(ctx, orc, reserve, waves):
    """"scan_lds_reserve" as the benchmark sets it leaves room for 16 waves; a larger one for 8; beyond that the four-wave kernel."""
    rng = np.random.default_rng(17)
    seqs = [_compressed(rng, int(rng.integers(300, 2 * BLOCK + 600))) for _ in range(40)]
    ctx.set_option("scan_lds_reserve", reserve)
    try:
        exp = _compare(ctx, orc, seqs, prefiltered=waves > 0)
        if waves:
            assert ctx.scan_info()["prefilter_waves"] == waves
    finally:
        ctx.set_option("scan_lds_reserve", 0)
    assert sum(len(e["minimizers"]) for e in exp) >= 100


# ---- the switch, and what keeps the four-wave kernels ---------------------------------------------------------------------------
def test_switch_off_gives_the_same_arrays(ctx, orc):
    rng = np.random.default_rng(19)
    seqs = _mixed(rng, 24)
    exp = _compare(ctx, orc, seqs)
    ctx.set_option("scan_prefilter", 0)
    try:
        _compare(ctx, orc, seqs, prefiltered=False)
    finally:
        ctx.set_option("scan_prefilter", 1)
    assert sum(len(e["minimizers"]) for e in exp) >= 40


def test_fall_backs_take_the_four_wave_kernel(ctx, orc):
    rng = np.random.default_rng(23)
    seqs = [_compressed(rng, int(rng.integers(300, BLOCK + 600))) for _ in range(12)]
    if not ctx.log2_bits:                    # a density whose bitmap is more than a quarter full (a forced geometry is used whatever its fill)
        exp = _compare(ctx, orc, seqs, density=0.02, prefiltered=False)
        assert ctx.scan_info()["bitmap_bits_set"] * 4 > 1 << 19 and sum(len(e["minimizers"]) for e in exp) >= 200
    for kw in (dict(k=13), dict(hpc=False)):
        exp = _compare(ctx, orc, seqs, prefiltered=False, **kw)
        assert sum(len(e["minimizers"]) for e in exp) >= 40
    ctx.set_option("scan_candidate_slack", 4)
    try:
        _compare(ctx, orc, seqs, prefiltered=False)
    finally:
        ctx.set_option("scan_candidate_slack", 0)
