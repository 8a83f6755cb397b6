"""Long reads cut into segments, one wave per segment (scan.hip, scan_fast_kernel<.., SEG>; csrc/segments_dev.hpp; "scan_segments").
A plain read of more than one segment is scanned as several views -- each owns the windows that start in its segment and reads one
tile on behind it -- and joined afterwards; the result must be what the read gives scanned whole, bit for bit.  Every case compares
read by read with the oracle (minimizers, positions, directions, flags, counts; with qualities also the per-minimizer quality and the
mean) and asserts mdbg_scan_info's "reads_segmented" EXACTLY: the plain reads longer than a segment whose every cut has l run starts
in the tile behind it (the rule of segments_dev.hpp, restated here in numpy), minus the reads the case builds to fall back.  Unless a
case says otherwise "scan_segments" is 2 (every eligible read) and "scan_segment_bases" 2048, so that reads of a few tiles are cut.
Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

from metamdbg_amd import synth

pytestmark = pytest.mark.gpu

K = 15
DENSITY = 0.005
TILE = 2048


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _context(prefilter=1, log2_bits=0):
    from metamdbg_amd import capi
    c = capi.Context(0)
    c.set_option("scan_prefilter", prefilter)
    c.set_option("scan_prefilter_log2_bits", log2_bits)
    c.set_option("scan_segments", 2)
    c.set_option("scan_segment_bases", TILE)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = _context()
    yield c
    c.close()


# the two kernel families: the pre-filtered variant (its own bitmap, and one of 1024 bits that passes every position) and the four-wave kernels
@pytest.fixture(scope="module", params=[(1, 0), (0, 0), (1, 10)], ids=["prefiltered", "four-wave", "bitmap10"])
def fctx(request):
    c = _context(*request.param)
    yield c
    c.close()


def _ascii(codes) -> bytes:
    return bytes(synth.CODE2ASCII[np.asarray(codes, dtype=np.int64)])


def _no_runs(rng, n):
    """n codes, no two neighbours equal."""
    return np.cumsum(np.concatenate([rng.integers(0, 4, 1), rng.integers(1, 4, n - 1)])) % 4 if n > 1 else rng.integers(0, 4, n)


def _with_runs(rng, raw_len) -> bytes:
    """A read of exactly raw_len bases, a third of them inside runs of two and three."""
    c = _no_runs(rng, raw_len)
    return _ascii(np.repeat(c, rng.choice([1, 1, 2, 3], len(c)))[:raw_len])


def _joined(parts, keep=()):
    """Run-free code arrays end to end, run-free: where two would meet in a run the first base of the later part is changed -- or, when
    that part is one of `keep` (indices; a planted window), the last base of the earlier one."""
    out = np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])
    at = 0
    for i, p in enumerate(parts[:-1]):
        at += len(p)
        if out[at] == out[at - 1]:
            if i + 1 in keep:
                assert i not in keep and len(p) >= 2
                out[at - 1] = next(c for c in range(4) if c != out[at - 2] and c != out[at])
            else:
                nxt = out[at + 1] if at + 1 < len(out) else -1
                out[at] = next(c for c in range(4) if c != out[at - 1] and c != nxt)
    assert not (out[1:] == out[:-1]).any()
    return out


def _segmentable(s: bytes, seg: int, k: int, hpc: bool) -> bool:
    """The rule of segments_dev.hpp: a plain read of more than one segment, every cut followed by a tile that holds l run starts or
    reaches the read's end."""
    n = len(s)
    if n <= seg or b"N" in s:
        return False
    a = np.frombuffer(s, dtype=np.uint8)
    start = np.ones(n, dtype=bool)
    if hpc:
        start[1:] = a[1:] != a[:-1]
    return all(cut + TILE >= n or int(start[cut:cut + TILE].sum()) >= k for cut in range(seg, n, seg))


def _flags(e) -> int:
    return (1 if e["low_complexity"] else 0) | (2 if e["low_quality"] else 0)


def _nan_eq(a, b) -> bool:
    return (np.isnan(a) and np.isnan(b)) or a == b


def _scan(ctx, seqs, quals=None, seg=TILE, mode=2, fall_back=0, k=K, hpc=True, check_segmented=True, **kw):
    """One mdbg_scan of the batch; asserts "reads_segmented".  Returns the host arrays."""
    ctx.set_option("scan_segments", mode)
    ctx.set_option("scan_segment_bases", seg)
    reads = ctx.reads_from_ascii(seqs, quals)
    m = ctx.scan(reads, K=k, hpc=hpc, **kw)
    h = m.to_host()
    m.free()
    reads.free()
    if check_segmented:
        want = sum(_segmentable(s, seg, k, hpc) for s in seqs) - fall_back if mode else 0
        assert ctx.scan_info()["reads_segmented"] == want, (ctx.scan_info(), want)
    assert len(h["offsets"]) == len(seqs) + 1
    return h


def _compare(ctx, orc, seqs, quals=None, k=K, density=DENSITY, hpc=True, min_read_quality=0.0, repetitive=None, **kw):
    """Scan with the read filters; every read against readSelection's record.  Returns the oracle's records."""
    h = _scan(ctx, seqs, quals, k=k, density=density, hpc=hpc, min_read_quality=min_read_quality, repetitive=repetitive, apply_read_filters=True, **kw)
    exp = []
    for i, s in enumerate(seqs):
        e = orc.read_selection(s, quals[i] if quals else None, K=k, density=density, hpc=hpc, min_read_quality=min_read_quality, repetitive=repetitive)
        a, b = int(h["offsets"][i]), int(h["offsets"][i + 1])
        where = (k, density, hpc, i, len(s), e["hpc_length"])
        assert int(h["flags"][i]) == _flags(e), where
        assert b - a == len(e["minimizers"]), where
        assert np.array_equal(h["minimizers"][a:b], e["minimizers"]) and np.array_equal(h["pos"][a:b], e["pos"]) \
            and np.array_equal(h["dir"][a:b], e["dir"]), where
        if quals:
            assert np.array_equal(h["qual"][a:b], e["qual"]), where
            assert _nan_eq(float(h["mean_quality"][i]), float(e["mean_quality"])), where
        exp.append(e)
    return exp


def _compare_parse(ctx, orc, seqs, trim, k=K, density=DENSITY, hpc=True, **kw):
    """Scan without the read filters, with or without the end trim; every read against MinimizerParser::parse."""
    h = _scan(ctx, seqs, k=k, density=density, hpc=hpc, apply_read_filters=False, no_end_trim=not trim, **kw)
    exp = []
    for i, s in enumerate(seqs):
        e = orc.minimizer_parse(s, k, density, hpc, trim=1 if trim else 0)
        a, b = int(h["offsets"][i]), int(h["offsets"][i + 1])
        assert (h["minimizers"][a:b].tolist(), h["pos"][a:b].tolist(), h["dir"][a:b].tolist()) == (list(e[0]), list(e[1]), list(e[2])), (trim, i, len(s))
        assert int(h["flags"][i]) == 0
        exp.append(e)
    return exp


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


def _plant_at(rng, window, at, length):
    """A run-free read of `length` bases with `window` at raw offset `at`."""
    parts = ([_no_runs(rng, at)] if at else []) + [window] + ([_no_runs(rng, length - at - len(window))] if length > at + len(window) else [])
    c = _joined(parts, keep=(1 if at else 0,))
    assert len(c) == length and np.array_equal(c[at: at + len(window)], window)
    return c


# ---- 1. lengths around the cuts -------------------------------------------------------------------------------------------------------
BOUNDARY_LENGTHS = [TILE * m + d for m in (1, 2, 3) for d in (-1, 0, 1, 14, 15, 16)]


def _boundary_batch(seed, with_q):
    rng = np.random.default_rng(seed)
    seqs = [_ascii(_no_runs(rng, n)) for n in BOUNDARY_LENGTHS] + [_with_runs(rng, n) for n in BOUNDARY_LENGTHS]
    quals = [bytes((rng.integers(2, 60, len(s)) + 33).astype(np.uint8)) for s in seqs] if with_q else None
    return seqs, quals


@pytest.mark.parametrize("hpc,k,seg,with_q", [(True, 15, 2048, False), (True, 15, 4096, False), (True, 13, 2048, False), (True, 13, 4096, False),
                                              (False, 15, 2048, False), (False, 13, 4096, False), (False, 15, 4096, True), (True, 15, 2048, True)])
def test_lengths_around_the_cuts(ctx, orc, hpc, k, seg, with_q):
    seqs, quals = _boundary_batch(11, with_q)
    exp = _compare(ctx, orc, seqs, quals, k=k, hpc=hpc, seg=seg)
    assert sum(len(s) > seg for s in seqs) >= 20 and sum(len(e["minimizers"]) for e in exp) >= 150


def test_lengths_around_the_cuts_both_families(fctx, orc):
    seqs, _ = _boundary_batch(12, False)
    for seg in (2048, 4096):
        _compare(fctx, orc, seqs, seg=seg)


# ---- 2. runs at a cut -------------------------------------------------------------------------------------------------------------------
def _with_run(rng, length, at, n):
    """A run-free read with a run of n bases at raw offset `at`."""
    c = _no_runs(rng, length)
    base = next(x for x in range(4) if x != c[at - 1] and (at + n >= length or x != c[at + n]))
    c[at: at + n] = base
    return _ascii(c)


@pytest.mark.parametrize("hpc", [True, False])
def test_runs_at_a_cut(ctx, orc, hpc):
    rng = np.random.default_rng(21)
    n = 4 * TILE + 300
    seqs = [_with_run(rng, n, TILE - 3, 7),             # starts 3 bases in front of a cut
            _with_run(rng, n, TILE - 9, 9),             # ends exactly on one
            _with_run(rng, n, 2 * TILE, 9),             # starts exactly on one
            _with_run(rng, n, 2 * TILE - 1, 2),         # the cut inside a run of two
            _with_run(rng, n, TILE, 2100),              # nothing but a run in the tile behind the cut: unsegmentable
            _with_run(rng, n, 1000, 5000),              # ... twice over
            _with_run(rng, n, TILE + 10, 2030),         # 10 + 1 + 8 run starts in that tile: enough for l = 15
            _with_run(rng, n, TILE + 10, 2035)]         # 10 + 1 + 3: one short
    verdicts = [_segmentable(s, TILE, K, hpc) for s in seqs]
    assert verdicts == ([True] * 4 + [False, False, True, False] if hpc else [True] * 8)
    exp = _compare(ctx, orc, seqs, hpc=hpc)
    # (a run of 2000 bases makes a read of 8500 low-complexity: those four select nothing under the read filters, so once more without)
    assert all(len(e["minimizers"]) >= 30 for e in exp[:4]) and [e["low_complexity"] for e in exp] == [False] * 4 + [True] * 4
    parsed = _compare_parse(ctx, orc, seqs, True, hpc=hpc)
    assert all(len(e[0]) >= 10 for e in parsed)


# ---- 3. a selected window across a cut ---------------------------------------------------------------------------------------------------
def _window_cases(windows):
    rng = np.random.default_rng(31)
    cases = [(cut - d, windows[(7 * d + cut) % len(windows)]) for cut in (TILE, 2 * TILE) for d in range(17)]
    return cases, [_ascii(_plant_at(rng, w, at, 3 * TILE + 100)) for at, w in cases]


def _check_windows(exp, cases):
    for e, (at, w) in zip(exp, cases):
        assert e["pos"].tolist().count(at) == 1, at                       # selected exactly once, where it was planted


def test_a_selected_window_across_a_cut(ctx, orc, selected_windows):
    cases, seqs = _window_cases(selected_windows)
    _check_windows(_compare(ctx, orc, seqs), cases)


def test_a_selected_window_across_a_cut_both_families(fctx, orc, selected_windows):
    cases, seqs = _window_cases(selected_windows)
    _check_windows(_compare(fctx, orc, seqs), cases)


# ---- 4. the end trim is the read's, not the view's ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trim", [True, False])
def test_end_trim_at_the_reads_ends_only(ctx, orc, selected_windows, trim):
    rng = np.random.default_rng(41)
    n = 3 * TILE
    w = [selected_windows[i] for i in (3, 14, 15, 92)]
    c = _joined([w[0], _no_runs(rng, TILE - K), w[1], _no_runs(rng, TILE - K), w[2], _no_runs(rng, TILE - 2 * K), w[3]], keep=(0, 2, 4, 6))
    assert len(c) == n and all(np.array_equal(c[at: at + K], x) for at, x in zip((0, TILE, 2 * TILE, n - K), w))
    (e,) = _compare_parse(ctx, orc, [_ascii(c)], trim)
    pos = list(e[1])
    assert TILE in pos and 2 * TILE in pos                        # the first window a view owns is kept
    assert (0 in pos) == (not trim) and (n - K in pos) == (not trim)      # the read's first and last l-mer only without the trim


# ---- 5. qualities ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [0, 1])
def test_quality_span_that_ends_in_the_next_segment(ctx, orc, selected_windows, window):
    """A selected window 8 bases in front of a cut whose last base is a run of three: its quality span ends in the next segment, on the
    run's last base (ReadSelection's span, [rle[pos], rle[pos + l])) or on its first (the correction scan's, [rle[pos], rle[pos + l - 1]])."""
    rng = np.random.default_rng(51)
    at = TILE - 8
    w = selected_windows[5]
    c = _plant_at(rng, w, at, 3 * TILE - 2)
    c = np.concatenate([c[:at + K], [c[at + K - 1]] * 2, c[at + K:]])           # the window's last base three times over
    s = _ascii(c)
    end = at + K - 1 + (0 if window else 2)                                     # the last raw base of the span
    seqs, quals = [], []
    for low_at in (end, end + 1):
        q = np.full(len(s), 40 + 33, dtype=np.uint8)
        q[low_at] = 3 + 33
        seqs.append(s)
        quals.append(bytes(q))
    assert end >= TILE and len(s) == 3 * TILE
    if window:
        h = _scan(ctx, seqs, quals, density=DENSITY, apply_read_filters=False, quality_window=1)
        exp = [orc.correction_scan(s_, q_, K=K, density=DENSITY, hpc=True) for s_, q_ in zip(seqs, quals)]
        for i, e in enumerate(exp):
            a, b = int(h["offsets"][i]), int(h["offsets"][i + 1])
            assert (h["minimizers"][a:b].tolist(), h["pos"][a:b].tolist(), h["dir"][a:b].tolist(), h["qual"][a:b].tolist()) == \
                (e["minimizers"].tolist(), e["pos"].tolist(), e["dir"].tolist(), e["qual"].tolist()), i
    else:
        exp = _compare(ctx, orc, seqs, quals)
    quality = [int(e["qual"][e["pos"].tolist().index(at)]) for e in exp]
    assert quality == [3, 40]                  # on the span's last base it shows, one base on it does not


def test_mean_quality_filter_on_segmented_reads(ctx, orc):
    rng = np.random.default_rng(53)
    seqs = [_with_runs(rng, 3 * TILE + 17 * i) for i in range(6)]
    quals = [bytes(np.full(len(s), (5 if i % 2 else 30) + 33, dtype=np.uint8)) for i, s in enumerate(seqs)]
    exp = _compare(ctx, orc, seqs, quals, min_read_quality=10.0)
    assert [e["low_quality"] for e in exp] == [False, True] * 3
    assert all(len(e["minimizers"]) == 0 for e in exp[1::2]) and all(len(e["minimizers"]) >= 10 for e in exp[0::2])


# ---- 6. complexity: one decision per read -----------------------------------------------------------------------------------------------------
def test_low_complexity_is_decided_once_per_read(ctx, orc):
    rng = np.random.default_rng(61)
    seqs = []
    for stretch in (1600, 2620, 8192):
        c = _no_runs(rng, 8192)
        at = 0 if stretch == 8192 else 1800
        c[at: at + stretch] = np.arange(stretch) % 2                 # ACAC...
        if at:                                                       # (keep the read run-free at the stretch's ends)
            c[at - 1] = next(x for x in (2, 3) if x != c[at - 2])
            c[at + stretch] = next(x for x in (2, 3) if x != c[at + stretch + 1])
        assert not (c[1:] == c[:-1]).any()
        seqs.append(_ascii(c))
    # ... and two short reads, low-complexity by the reference's score, whose 2-mer bound is close to its threshold (units of the squared
    # 2-mer counts; the kernel's sum is 4 x that less a constant).  Word 63, the last of the first segment, is counted by the view BEHIND
    # the cut; left out, it takes 2 (sq - 64) from the sum.
    #   * 2144 bases of period 8 with 700 of period 4 across base 2048: the bound exceeds its threshold by 480, word 63 (sq = 256) carries
    #     384 -- the verdict survives its loss;
    #   * 2084 bases of period 8 with 126 A from base 1940: the reference's score is 5.0046 (> 5), the bound exceeds its threshold by 828
    #     and word 63, all A (sq = 1024), carries 1920 -- without it the read is no suspect, keeps its minimizers and loses its flag.  The
    #     complexity score is taken on the raw bases, so a homopolymer word weighs most.
    bg = "ACGTCATG" * 400
    seqs.append((bg[:1400] + "ACGT" * 175 + "ACGTCATG" * 10)[:2144].encode())
    seqs.append((bg[:1940] + "A" * 126 + bg[2066:2084]).encode())
    assert len(seqs[-1]) == 2084
    for hpc in (True, False):
        exp = _compare(ctx, orc, seqs, hpc=hpc)
        assert [e["low_complexity"] for e in exp] == [False, True, True, True, True]
        assert len(exp[4]["minimizers"]) == 0
        assert len(exp[0]["minimizers"]) >= 10 and len(exp[1]["minimizers"]) == 0


# ---- 7. the repetitive list ----------------------------------------------------------------------------------------------------------------
def test_repetitive_minimizers_in_a_segmented_read(ctx, orc):
    rng = np.random.default_rng(71)
    seqs = [_with_runs(rng, 5 * TILE + 77), _ascii(_no_runs(rng, 3 * TILE))]
    plain = orc.read_selection(seqs[0], None, K=K, density=DENSITY, hpc=True)
    rep = [int(plain["minimizers"][i]) for i in (1, len(plain["minimizers"]) // 2, len(plain["minimizers"]) - 2)]
    exp = _compare(ctx, orc, seqs, repetitive=rep)
    assert len(exp[0]["minimizers"]) == len(plain["minimizers"]) - 3 and not set(rep) & set(exp[0]["minimizers"].tolist())


# ---- 8. a mixed batch: order, reads that stay whole, a read that falls back ----------------------------------------------------------------------
SEG_MIXED = 3 * TILE


def _mixed_batch(windows):
    """40 reads: short ones, segmented ones, two with an N (they stay whole), and one of 1000 selected windows end to end -- 409 in every
    segment of 6144 bases, more than either stage holds (384, 176): its views outgrow the stage and the whole read falls back."""
    rng = np.random.default_rng(81)
    seqs = []
    for i in range(40):
        if i in (9, 30):
            s = bytearray(_with_runs(rng, 3 * SEG_MIXED + 100 * i))
            s[SEG_MIXED + 5] = ord("N")
            seqs.append(bytes(s))
        elif i == 17:
            seqs.append(_ascii(_planted(windows, 1000, 11)))
        elif i % 3 == 0:
            seqs.append(_with_runs(rng, int(rng.integers(SEG_MIXED + 1, 4 * SEG_MIXED))))
        else:
            seqs.append(_with_runs(rng, int(rng.integers(20, SEG_MIXED))))
    return seqs


@pytest.mark.parametrize("per_wave", [1, 2])
def test_mixed_batch_keeps_the_read_order(fctx, orc, selected_windows, per_wave):
    seqs = _mixed_batch(selected_windows)
    assert sum(_segmentable(s, SEG_MIXED, K, True) for s in seqs) == 12 + 1 and sum(b"N" in s for s in seqs) == 2
    fctx.set_option("scan_reads_per_wave", per_wave)
    try:
        exp = _compare(fctx, orc, seqs, seg=SEG_MIXED, fall_back=1)
    finally:
        fctx.set_option("scan_reads_per_wave", 2)
    assert len(exp[17]["minimizers"]) >= 990 and sum(len(e["minimizers"]) for e in exp) >= 1500


# ---- 10. automatic mode, default options ------------------------------------------------------------------------------------------------------
# Eight reads of 200 kb: the average is far above the 64 kb up to which a batch takes the block-structured kernels in bump mode.  With
# qualities such a batch is the general kernel's today (no block-kernel launch at all); without, the general path scans it with a
# block-structured kernel in its padded-slot form, one wave a read, which mdbg_scan_info counts as one block launch -- so the
# statement "no block-kernel launch with "scan_segments" 0" is asserted where it holds today, on the reads with qualities.
@pytest.fixture(scope="module")
def long_reads():
    rng = np.random.default_rng(101)
    seqs = [_ascii(rng.integers(0, 4, 200_000)) for _ in range(8)]
    return seqs, [bytes((rng.integers(2, 60, len(s)) + 33).astype(np.uint8)) for s in seqs]


@pytest.fixture(scope="module")
def long_reads_expected(orc, long_reads):
    seqs, quals = long_reads
    return {with_q: [orc.read_selection(s, q if with_q else None, K=K, density=DENSITY, hpc=True) for s, q in zip(seqs, quals)] for with_q in (False, True)}


@pytest.mark.parametrize("with_q", [True, False])
@pytest.mark.parametrize("mode,segmented", [(-1, 8), (0, 0), (2, 8)])          # (2 includes the automatic case)
def test_automatic_mode_takes_a_batch_of_long_reads(orc, long_reads, long_reads_expected, mode, segmented, with_q):
    from metamdbg_amd import capi
    c = capi.Context(0)                   # every other option at its default
    try:
        c.set_option("scan_segments", mode)
        c.set_option("scan_segment_bases", -1)
        before = c.scan_info()
        reads = c.reads_from_ascii(long_reads[0], long_reads[1] if with_q else None)
        m = c.scan(reads, K=K, density=DENSITY, hpc=True)
        h = m.to_host()
        m.free()
        reads.free()
        after = c.scan_info()
        assert after["reads_segmented"] == segmented, after
        launched = after["prefiltered_launches"] + after["block_launches"] - before["prefiltered_launches"] - before["block_launches"]
        if segmented:
            assert launched >= 1, (before, after)
            assert after["last_prefiltered"] == (0 if with_q else 1)         # segments of 16384 bases are the pre-filtered variant's where it applies
        elif with_q:
            assert launched == 0, (before, after)
        else:                 # the routing as before: the general path's one launch of a block-structured kernel in its padded-slot form
            assert launched == 1 and after["prefiltered_launches"] == before["prefiltered_launches"], (before, after)
        for i, e in enumerate(long_reads_expected[with_q]):
            a, b = int(h["offsets"][i]), int(h["offsets"][i + 1])
            assert int(h["flags"][i]) == 0 and b - a == len(e["minimizers"]) >= 500
            assert np.array_equal(h["minimizers"][a:b], e["minimizers"]) and np.array_equal(h["pos"][a:b], e["pos"]) and np.array_equal(h["dir"][a:b], e["dir"])
            if with_q:
                assert np.array_equal(h["qual"][a:b], e["qual"]) and _nan_eq(float(h["mean_quality"][i]), float(e["mean_quality"]))
    finally:
        c.close()


def test_automatic_mode_leaves_a_batch_of_short_reads_alone(orc):
    from metamdbg_amd import capi
    rng = np.random.default_rng(103)
    seqs = [_ascii(rng.integers(0, 4, 10_000)) for _ in range(12)]
    c = capi.Context(0)
    try:
        c.set_option("scan_segments", 1)
        reads = c.reads_from_ascii(seqs)
        m = c.scan(reads, K=K, density=DENSITY, hpc=True)
        h = m.to_host()
        m.free()
        reads.free()
        assert c.scan_info()["reads_segmented"] == 0
        e = orc.read_selection(seqs[3], None, K=K, density=DENSITY, hpc=True)
        a, b = int(h["offsets"][3]), int(h["offsets"][4])
        assert np.array_equal(h["minimizers"][a:b], e["minimizers"]) and np.array_equal(h["pos"][a:b], e["pos"])
    finally:
        c.close()


# ---- 11. a contig ------------------------------------------------------------------------------------------------------------------------------
def test_a_contig_of_three_megabases(orc):
    from metamdbg_amd import capi
    rng = np.random.default_rng(111)
    s = _ascii(rng.integers(0, 4, 3_000_000))
    c = capi.Context(0)
    try:
        c.set_option("scan_segments", 1)          # automatic; the segment length stays the default
        reads = c.reads_from_ascii([s])
        m = c.scan(reads, K=K, density=DENSITY, hpc=True, apply_read_filters=False, no_end_trim=True)
        h = m.to_host()
        m.free()
        reads.free()
        assert c.scan_info()["reads_segmented"] == 1
        e = orc.minimizer_parse(s, K, DENSITY, True, trim=0)
        assert len(e[0]) >= 10_000 and int(h["offsets"][1]) == len(e[0])
        assert np.array_equal(h["minimizers"], np.asarray(e[0], dtype=np.uint32)) and np.array_equal(h["pos"], np.asarray(e[1], dtype=np.uint32)) \
            and np.array_equal(h["dir"], np.asarray(e[2], dtype=np.uint8))
    finally:
        c.close()


# ---- the options ------------------------------------------------------------------------------------------------------------------------------
def test_option_values(ctx):
    from metamdbg_amd import capi
    for bad in (1, 2047, 3000, 2048 * 3 + 1):
        with pytest.raises(capi.MdbgError):
            ctx.set_option("scan_segment_bases", bad)
    with pytest.raises(capi.MdbgError):
        ctx.set_option("scan_segments", 3)
    for ok in (2048, 6144, 16384, 0, -5):
        ctx.set_option("scan_segment_bases", ok)
    ctx.set_option("scan_segment_bases", TILE)
