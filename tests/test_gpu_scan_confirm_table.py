"""The selected-key table of the pre-filtered scan's confirmation (scan.hip, confirm; csrc/prefilter.hpp): a candidate's exact verdict
from one 16-byte load instead of the full hash.  Every case read by read against the oracle -- values, positions, directions, flags,
counts -- in three forms of one context: the table at its own geometry (2^16 buckets, none overflowed at density 0.005), a table of
2^13 buckets (half of them marked, so that looked-up verdicts and hashed ones mix inside one round of 64 candidates) and the table
switched off (every candidate hashed, as before).  mdbg_scan_confirm_info says which path ran.
Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

from metamdbg_amd import synth

pytestmark = pytest.mark.gpu

K = 15
DENSITY = 0.005
BLOCK = 2048                     # positions of a block
FORMS = {"table16": (1, 0), "table13": (1, 13), "hashed": (0, 0)}
OVERFLOWED_16 = {0.005: 0, 0.01: 9, 0.002: 0}        # buckets of more than seven keys: tests/host/test_confirm_table.cpp


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _context(form, log2_bits=0):
    from metamdbg_amd import capi
    c = capi.Context(0)
    c.set_option("scan_prefilter", 1)
    c.set_option("scan_prefilter_log2_bits", log2_bits)
    c.set_option("scan_confirm_table", FORMS[form][0])
    c.set_option("scan_confirm_table_log2_buckets", FORMS[form][1])
    c.form = form
    return c


@pytest.fixture(scope="module", params=list(FORMS))
def ctx(request):
    c = _context(request.param)
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


def _expected(orc, s, density):
    """The oracle's record of a read, computed once per (read, density) and shared by the forms."""
    key = (s, density)
    if key not in _EXPECTED:
        _EXPECTED[key] = orc.read_selection(s, None, K=K, density=density, hpc=True)
    return _EXPECTED[key]


def _compare(ctx, orc, seqs, density=DENSITY, prefiltered=True):
    """Scan; every read against readSelection's record; which kernel and which confirmation ran.  Returns the oracle's records."""
    before = ctx.scan_info()
    reads = ctx.reads_from_ascii(seqs)
    m = ctx.scan(reads, K=K, density=density, hpc=True, apply_read_filters=True)
    h = m.to_host()
    m.free()
    reads.free()
    after, table = ctx.scan_info(), ctx.scan_confirm_info()
    assert after["prefiltered_launches"] == before["prefiltered_launches"] + (1 if prefiltered else 0), (before, after)
    want_table = prefiltered and FORMS[ctx.form][0] == 1
    assert table["last_by_table"] == (1 if want_table else 0), (ctx.form, table)
    if want_table:
        assert table["table_buckets"] == 1 << (FORMS[ctx.form][1] or 16), table
    assert len(h["offsets"]) == len(seqs) + 1
    exp = []
    for i, s in enumerate(seqs):
        e = _expected(orc, s, density)
        a, b = int(h["offsets"][i]), int(h["offsets"][i + 1])
        where = (ctx.form, density, i, len(s), e["hpc_length"])
        assert int(h["flags"][i]) == (1 if e["low_complexity"] else 0), where
        assert b - a == len(e["minimizers"]), where
        assert np.array_equal(h["minimizers"][a:b], e["minimizers"]) and np.array_equal(h["pos"][a:b], e["pos"]) \
            and np.array_equal(h["dir"][a:b], e["dir"]), where
        exp.append(e)
    return exp


# ---- compressed lengths around l, the block, the tail and the tail's spans ------------------------------------------------------
def test_lengths_at_every_border(ctx, orc):
    rng = np.random.default_rng(31)
    lengths = [K - 1, K, K + 1, 2047, 2048, 2048 + K, 2 * BLOCK + 90]
    # a read of compressed length c has c - l positions followed by a base: tails of exactly 64 P and 64 P + 1 positions, alone and behind a block
    npos = [64 * 5, 64 * 5 + 1, 64 * 32, BLOCK + 64 * 7, BLOCK + 64 * 7 + 1, 64, 65]
    seqs = [_compressed(rng, c) for c in lengths] + [_compressed(rng, p + K) for p in npos]
    exp = _compare(ctx, orc, seqs)
    assert [e["hpc_length"] for e in exp] == lengths + [p + K for p in npos]
    assert all(len(e["minimizers"]) == 0 for e in exp[:3]) and all(len(e["minimizers"]) >= 3 for e in exp[3:7])


# ---- batch sizes around one workgroup's chunk, at 1 and 2 reads a wave ------------------------------------------------------------
@pytest.mark.parametrize("n,per_wave", [(1, 1), (16, 1), (17, 1), (33, 1), (1, 2), (16, 2), (17, 2), (33, 2)])
def test_batch_sizes(ctx, orc, n, per_wave):
    rng = np.random.default_rng(200 + n)           # (the same reads at 1 and 2 a wave: one oracle run)
    lengths = [3 * BLOCK + 500, K + 1, BLOCK + K, 700, 2 * BLOCK + 90, 40]
    seqs = [_compressed(rng, lengths[i % len(lengths)] if i < len(lengths) else int(rng.integers(1, 2 * BLOCK))) for i in range(n)]
    ctx.set_option("scan_reads_per_wave", per_wave)
    try:
        exp = _compare(ctx, orc, seqs)
    finally:
        ctx.set_option("scan_reads_per_wave", 0)
    assert sum(len(e["minimizers"]) for e in exp) >= 20


# ---- planted reads ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def selected_windows(orc):
    """Compressed 15-mers the oracle selects, as they stood in a random run-free sequence (codes, reading order)."""
    rng = np.random.default_rng(2027)
    c = _no_runs(rng, 200_000)
    _, pos, _ = orc.minimizer_parse(_ascii(c), K, DENSITY, True)
    assert len(pos) >= 600
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


def test_rounds_full_of_selected_windows_and_rounds_without_any(ctx, orc, selected_windows):
    """A read of selected windows end to end: every 15th position of a block is selected (136) and the bitmap passes 8.65 % of the
    others, about 300 candidates -- more than one pass lists, so the block takes two, and a round of 64 candidates holds some thirty
    selected keys.  Beside it reads in which the oracle selects nothing: each of their rounds ends without a survivor."""
    rng = np.random.default_rng(37)
    planted = [_ascii(_planted(selected_windows, n, 41 * n)) for n in (140, 11)]          # 2100 and 165 positions
    none = []
    while len(none) < 3:
        s = _compressed(rng, 150)
        if len(_expected(orc, s, DENSITY)["minimizers"]) == 0:
            none.append(s)
    seqs = [none[0], planted[0], none[1], planted[1], none[2]]
    exp = _compare(ctx, orc, seqs)
    assert len(exp[1]["minimizers"]) >= 138          # with 0.0865 x 1900 false positives more than the LIST_CAP = 224 one pass lists
    assert len(exp[3]["minimizers"]) >= 9
    assert all(len(exp[i]["minimizers"]) == 0 for i in (0, 2, 4))


# ---- every position looked up: the 1024-bit bitmap, all of whose bits are set ---------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_every_position_is_a_candidate(orc, form, selected_windows):
    """With "scan_prefilter_log2_bits" = 10 all 2048 positions of a block reach the confirmation, in ten passes of four rounds: keys of
    empty buckets, of full ones and of marked ones, and lanes without a listed position in the last round."""
    rng = np.random.default_rng(41)
    seqs = [_compressed(rng, c) for c in (2 * BLOCK + 90, K + 1, BLOCK + K, 64 * 5 + 1 + K, 700)] + [_ascii(_planted(selected_windows, 140, 3))]
    c = _context(form, log2_bits=10)
    try:
        exp = _compare(c, orc, seqs)
        assert c.scan_info()["bitmap_bits_set"] == 1024
    finally:
        c.close()
    assert sum(len(e["minimizers"]) for e in exp) >= 150


# ---- the table's cache: rebuilt with the bitmap, one per context --------------------------------------------------------------------
def test_densities_in_turn_and_two_contexts_together(ctx, orc):
    """0.005f, then 0.002f and 0.01f on the same context: a table kept from the density before would select the wrong keys (0.002f:
    too many, 0.01f: too few).  At 0.01f nine buckets of the 2^16 hold more than seven keys and ask the hash."""
    rng = np.random.default_rng(43)
    seqs = [_compressed(rng, int(rng.integers(500, 2 * BLOCK + 600))) for _ in range(12)]
    other = _context(ctx.form)
    try:
        _compare(ctx, orc, seqs, density=0.003)                            # whatever ran before: the context's table is another density's now
        built = ctx.scan_confirm_info()["tables_built"]
        counts = []
        for density in (0.005, 0.002, 0.002, 0.01, 0.005):
            exp = _compare(ctx, orc, seqs, density=density)
            _compare(other, orc, seqs, density=0.003)                    # another context, another key, alive beside it
            counts.append(sum(len(e["minimizers"]) for e in exp))
            if ctx.form == "table16":
                assert ctx.scan_confirm_info()["table_overflowed"] == OVERFLOWED_16[density], density
            elif ctx.form == "table13":
                assert 0 < ctx.scan_confirm_info()["table_overflowed"] <= 8192
        table = FORMS[ctx.form][0]
        assert ctx.scan_confirm_info()["tables_built"] == built + 4 * table          # rebuilt when the density changes, kept when it does not
        assert other.scan_confirm_info()["tables_built"] == table
        assert counts[3] > counts[0] == counts[4] > counts[1] == counts[2] > 10
    finally:
        other.close()


# ---- the 8-wave instantiation, and the switches ----------------------------------------------------------------------------------
def test_eight_waves_under_a_large_reserve(ctx, orc):
    rng = np.random.default_rng(47)
    seqs = [_compressed(rng, int(rng.integers(300, 2 * BLOCK + 600))) for _ in range(20)]
    ctx.set_option("scan_lds_reserve", 60000)
    try:
        exp = _compare(ctx, orc, seqs)
        assert ctx.scan_info()["prefilter_waves"] == 8
    finally:
        ctx.set_option("scan_lds_reserve", 0)
    assert sum(len(e["minimizers"]) for e in exp) >= 50


def test_without_the_prefilter_the_table_is_neither_built_nor_used(orc):
    rng = np.random.default_rng(53)
    seqs = [_compressed(rng, int(rng.integers(300, BLOCK + 600))) for _ in range(8)]
    c = _context("table16")
    try:
        c.set_option("scan_prefilter", 0)
        _compare(c, orc, seqs, prefiltered=False)
        assert c.scan_confirm_info() == {"tables_built": 0, "table_buckets": 0, "table_overflowed": 0, "last_by_table": 0}
        c.set_option("scan_prefilter", 1)
        _compare(c, orc, seqs)
        assert c.scan_confirm_info() == {"tables_built": 1, "table_buckets": 65536, "table_overflowed": 0, "last_by_table": 1}
        c.set_option("scan_confirm_table", 0)          # the switch on a context that has a table: the launch hashes
        c.form = "hashed"
        _compare(c, orc, seqs)
        assert c.scan_confirm_info()["tables_built"] == 1
    finally:
        c.close()


def test_option_range():
    from metamdbg_amd import capi
    c = capi.Context(0)
    try:
        for bad in (9, 17, -1):
            with pytest.raises(Exception):
                c.set_option("scan_confirm_table_log2_buckets", bad)
        for good in (10, 16, 0):
            c.set_option("scan_confirm_table_log2_buckets", good)
    finally:
        c.close()
