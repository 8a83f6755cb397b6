"""The pre-filtered scan variant stages its rows from the confirmation round (scan.hip, scan_fast_kernel<.., PFW>, confirm): the lane that
confirms a candidate writes the finished row -- value, position, direction -- to the stage at its rank in the round's ballot; the
variant has no emit and no materialise, and releases its ring after every block.  Every case compares read by read with the oracle:
values, positions, directions, flags and counts, and mdbg_scan_info shows that the variant ran.  Each case runs with the bitmap of 2^19
bits and with "scan_prefilter_log2_bits" 10, a bitmap of 1024 bits, all set, that sends every position of a block through the
confirmation in ten passes of its list.  Reads have three blocks or fewer and batches 33 reads or fewer (one case, named, has a read
of 40 kb).  profiles/direct_rows_mutation_checks.txt lists the value-only mutants of the round these cases were run against.
Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

from tests.test_gpu_scan_prefilter import BLOCK, DENSITY, K, STAGE, _ascii, _compressed, _expected, _no_runs, _planted

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _context(log2_bits, table=0, log2_buckets=0):
    from metamdbg_amd import capi
    c = capi.Context(0)
    c.set_option("scan_prefilter", 1)
    c.set_option("scan_prefilter_log2_bits", log2_bits)
    c.set_option("scan_confirm_table", table)
    c.set_option("scan_confirm_table_log2_buckets", log2_buckets)
    c.log2_bits, c.table = log2_bits, table
    return c


@pytest.fixture(scope="module", params=[0, 10], ids=["bitmap19", "bitmap10"])
def ctx(request):
    c = _context(request.param)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[(0, 16), (0, 13), (10, 16), (10, 13)], ids=["bitmap19-2^16", "bitmap19-2^13", "bitmap10-2^16", "bitmap10-2^13"])
def tctx(request):
    c = _context(request.param[0], 1, request.param[1])
    yield c
    c.close()


@pytest.fixture(scope="module")
def selected_windows(orc):
    """Compressed 15-mers the oracle selects, as they stood in a random run-free sequence (codes, reading order)."""
    rng = np.random.default_rng(2026)
    c = _no_runs(rng, 300_000)
    _, pos, _ = orc.minimizer_parse(_ascii(c), K, DENSITY, True)
    assert len(pos) >= 1000
    return [c[p: p + K] for p in pos]


def _mixed(rng, n):
    """n reads from shorter than l to two blocks and a tail, compressed."""
    lengths = [K - 3, K, K + 1, 2 * BLOCK + 500, 40, BLOCK + K, 700, BLOCK + 90]
    return [_compressed(rng, lengths[i % len(lengths)] if i < len(lengths) else int(rng.integers(1, 2 * BLOCK + 1000))) for i in range(n)]


def _scan(ctx, seqs, variant=True, **kw):
    """One mdbg_scan of the batch by the variant (mdbg_scan_info says so); the host arrays."""
    before = ctx.scan_info()
    reads = ctx.reads_from_ascii(seqs)
    m = ctx.scan(reads, K=K, density=DENSITY, hpc=True, **kw)
    h = m.to_host()
    m.free()
    reads.free()
    after = ctx.scan_info()
    if variant:
        assert after["prefiltered_launches"] == before["prefiltered_launches"] + 1 and after["block_launches"] == before["block_launches"], (before, after)
        assert after["bitmap_log2_bits"] == (ctx.log2_bits or 19)
        assert ctx.scan_confirm_info()["last_by_table"] == ctx.table
    assert len(h["offsets"]) == len(seqs) + 1
    return h


def _rows(h, i):
    a, b = int(h["offsets"][i]), int(h["offsets"][i + 1])
    return h["minimizers"][a:b].tolist(), h["pos"][a:b].tolist(), h["dir"][a:b].tolist()


def _compare(ctx, orc, seqs, repetitive=None, variant=True):
    """Scan with the read filters and the end trim; every read against readSelection's record.  Returns the oracle's records."""
    h = _scan(ctx, seqs, variant, apply_read_filters=True, repetitive=repetitive)
    exp = []
    for i, s in enumerate(seqs):
        e = _expected(orc, s, K, DENSITY, True) if repetitive is None else orc.read_selection(s, None, K=K, density=DENSITY, hpc=True, repetitive=repetitive)
        where = (i, len(s), e["hpc_length"], len(e["minimizers"]))
        assert int(h["flags"][i]) == (1 if e["low_complexity"] else 0), where
        assert int(h["offsets"][i + 1]) - int(h["offsets"][i]) == len(e["minimizers"]), where
        assert _rows(h, i) == (e["minimizers"].tolist(), e["pos"].tolist(), e["dir"].tolist()), where
        exp.append(e)
    return exp


def _compare_untrimmed(ctx, orc, seqs):
    """Scan without the read filters and without the end trim; every read against MinimizerParser::parse with _trimBps 0."""
    h = _scan(ctx, seqs, apply_read_filters=False, no_end_trim=True)
    exp = []
    for i, s in enumerate(seqs):
        e = orc.minimizer_parse(s, K, DENSITY, True, trim=0)
        assert _rows(h, i) == (list(e[0]), list(e[1]), list(e[2])), (i, len(s), len(e[0]))
        assert int(h["flags"][i]) == 0
        exp.append(e)
    return exp


# ---- length borders: a round of one, a full round, a round and one more; a block, the block and one position of tail ----------------
NPOS = [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1, 2 * BLOCK + 64, 2 * BLOCK + BLOCK - 1]


@pytest.mark.parametrize("trim", [True, False], ids=["end_trim", "no_end_trim"])
def test_length_borders(ctx, orc, trim):
    """With the end trim a read of compressed length c has c - l positions (each followed by a base), without it c - l + 1."""
    rng = np.random.default_rng(41)
    seqs = [_compressed(rng, p + K if trim else p + K - 1) for p in NPOS]
    if trim:
        exp = _compare(ctx, orc, seqs)
        assert [e["hpc_length"] - K for e in exp] == NPOS
        counts = [len(e["minimizers"]) for e in exp]
    else:
        counts = [len(e[0]) for e in _compare_untrimmed(ctx, orc, seqs)]
    assert all(c == 0 for c in counts[:2]) and all(c >= 3 for c in counts[5:]) and sum(counts) >= 60


# ---- the stage's cap: reads of exactly 175, 176 and 177 minimizers -------------------------------------------------------------------
_TRIMMED = {}


def _trimmed_to_count(orc, windows, target, length, seed):
    """A run-free read of `length` bases that the oracle gives exactly `target` minimizers: planted windows in front, the same random
    rest behind them, and one planted window after the other taken away (the rest grows by its 15 bases) until the oracle says so."""
    key = (target, length, seed)
    if key not in _TRIMMED:
        rest = _no_runs(np.random.default_rng(seed), length)
        for n in range(target + 2, target - 40, -1):
            head = _planted(windows, n, seed)
            tail = rest[:length - len(head)].copy()
            if tail[0] == head[-1]:
                tail[0] = next(c for c in range(4) if c != head[-1] and c != tail[1])
            s = _ascii(np.concatenate([head, tail]))
            if len(_expected(orc, s, K, DENSITY, True)["minimizers"]) == target:
                _TRIMMED[key] = s
                break
        else:
            raise AssertionError(key)
    return _TRIMMED[key]


# (length, seed): one block and a tail of 900 positions; two blocks and a tail of 40 -- seeds at which the oracle reaches all three counts
CAP_READS = {"tail": (BLOCK + 900 + K, 6), "block": (2 * BLOCK + 40 + K, 3)}


@pytest.mark.parametrize("where", ["tail", "block"])
def test_reads_at_the_stage_cap(ctx, orc, selected_windows, where):
    """175 and 176 rows fit the stage, the 177th makes the read outgrow it (the host re-runs it by its exact count).  "tail": the 176th
    row falls in the tail behind one block.  "block": it falls in the second of two full blocks, in front of a tail of 40 positions."""
    length, seed = CAP_READS[where]
    seqs = [_trimmed_to_count(orc, selected_windows, t, length, seed) for t in (STAGE - 1, STAGE, STAGE + 1)]
    plain = _compressed(np.random.default_rng(43), 900)
    exp = _compare(ctx, orc, [seqs[0], plain, seqs[1], seqs[2], plain])
    assert [len(e["minimizers"]) for e in (exp[0], exp[2], exp[3])] == [STAGE - 1, STAGE, STAGE + 1]
    for e in (exp[2], exp[3]):
        p176 = int(e["pos"][STAGE - 1])
        assert (BLOCK <= p176 < e["hpc_length"] - K) if where == "tail" else (BLOCK <= p176 < 2 * BLOCK), (where, p176)


# ---- several rounds ------------------------------------------------------------------------------------------------------------------
def test_rounds_with_many_survivors(ctx, orc, selected_windows):
    """A block with more than 128 planted selected windows: under either bitmap its candidates take more than one pass, and rounds of 64
    listed positions hold several selected ones each -- up to five under the 1024-bit bitmap, most of them under the real one."""
    codes = _planted(selected_windows, 150, 900)
    exp = _compare(ctx, orc, [_ascii(codes), _ascii(codes[K * 3:])])
    for e in exp:
        in_block = int((e["pos"] < BLOCK).sum())
        assert 128 < in_block <= len(e["minimizers"]) <= STAGE


def test_rounds_without_survivors_between_rounds_with_one(ctx, orc):
    """A plain random read: a block selects about ten positions; under the 1024-bit bitmap it lists all 2048 in 32 rounds, most of which
    have no survivor."""
    rng = np.random.default_rng(47)
    seqs = [_ascii(_no_runs(rng, 2 * BLOCK + 700)), _compressed(rng, BLOCK + 40)]
    exp = _compare(ctx, orc, seqs)
    assert 10 <= len(exp[0]["minimizers"]) <= 2 * BLOCK // 64


# ---- the trimmed first position ------------------------------------------------------------------------------------------------------
def test_read_whose_first_window_is_selected(ctx, orc, selected_windows):
    rng = np.random.default_rng(53)
    rest = _no_runs(rng, 500)
    w = selected_windows[7]
    codes = np.concatenate([w, rest[1:] if rest[0] == w[-1] else rest])
    s = _ascii(codes)
    exp = _compare(ctx, orc, [s, s[:K + 1], s[:K]])
    assert all(0 not in e["pos"].tolist() for e in exp)                                  # Kmer.hpp:1395
    assert len(exp[1]["minimizers"]) == 0 and len(exp[2]["minimizers"]) == 0
    untrimmed = _compare_untrimmed(ctx, orc, [s, s[:K + 1], s[:K]])
    assert all(e[1][0] == 0 for e in untrimmed)                                          # ... and selected where nothing is trimmed


# ---- the repetitive list ---------------------------------------------------------------------------------------------------------------
def test_repetitive_values_leave_the_other_rows_where_they_are(ctx, orc, selected_windows):
    rng = np.random.default_rng(59)
    seqs = [_compressed(rng, 2 * BLOCK + 300), _ascii(_planted(selected_windows, 140, 77)), _compressed(rng, 700), _ascii(_no_runs(rng, BLOCK + K))]
    plain = [_expected(orc, s, K, DENSITY, True) for s in seqs]
    values = np.unique(np.concatenate([e["minimizers"] for e in plain]))
    rep = values[::3].astype(np.uint32)
    assert len(rep) >= 50
    exp = _compare(ctx, orc, seqs, repetitive=rep)
    for e, p in zip(exp, plain):
        keep = ~np.isin(p["minimizers"], rep)
        assert 0 < int(keep.sum()) < len(keep)
        assert np.array_equal(e["minimizers"], p["minimizers"][keep]) and np.array_equal(e["pos"], p["pos"][keep]) and np.array_equal(e["dir"], p["dir"][keep])


# ---- views of a long read ----------------------------------------------------------------------------------------------------------------
def test_one_long_read_in_segments(ctx, orc):
    """One read of 40 kb under "scan_segments" 2: its views are scanned by the SEG instantiation of the variant and joined."""
    rng = np.random.default_rng(61)
    c = _no_runs(rng, 40_000)
    s = _ascii(np.repeat(c, rng.choice([1, 1, 2, 3], len(c)))[:40_000])
    ctx.set_option("scan_segments", 2)
    try:
        exp = _compare(ctx, orc, [s])
        assert ctx.scan_info()["reads_segmented"] == 1
    finally:
        ctx.set_option("scan_segments", 1)
    assert len(exp[0]["minimizers"]) >= 60


# ---- the selected-key table ----------------------------------------------------------------------------------------------------------
def test_rows_from_the_confirm_table(tctx, orc, selected_windows):
    """2^16 buckets answer every key themselves; 2^13 buckets send many to the hash, within their round."""
    rng = np.random.default_rng(67)
    seqs = _mixed(rng, 9) + [_ascii(_planted(selected_windows, 150, 300)), _trimmed_to_count(orc, selected_windows, STAGE + 1, *CAP_READS["block"])]
    exp = _compare(tctx, orc, seqs)
    info = tctx.scan_confirm_info()
    assert info["last_by_table"] == 1 and (info["table_overflowed"] > 0) == (info["table_buckets"] < 65536), info
    assert sum(len(e["minimizers"]) for e in exp) >= 300


# ---- batches and waves -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 16, 17, 33])
def test_batch_sizes(ctx, orc, n):
    rng = np.random.default_rng(70 + n)
    seqs = [_compressed(rng, 2 * BLOCK + 500)] if n == 1 else _mixed(rng, n)
    exp = _compare(ctx, orc, seqs)
    assert sum(len(e["minimizers"]) for e in exp) >= 10


def test_eight_waves(ctx, orc, selected_windows):
    """"scan_lds_reserve" 60000 leaves room for the 8-wave form."""
    rng = np.random.default_rng(79)
    seqs = _mixed(rng, 17) + [_ascii(_planted(selected_windows, 150, 40))]
    ctx.set_option("scan_lds_reserve", 60000)
    try:
        exp = _compare(ctx, orc, seqs)
        assert ctx.scan_info()["prefilter_waves"] == 8
    finally:
        ctx.set_option("scan_lds_reserve", 0)
    assert sum(len(e["minimizers"]) for e in exp) >= 150
