"""The persistent launch of the pre-filtered scan (scan.hip, scan_fast_kernel<.., PFW>; scan_plan.hpp; "scan_persistent"): as many
workgroups as CUs, every wave drawing runs of R consecutive reads from one 64-bit counter in device memory until it is used up.  Every
case against the oracle read by read -- values, positions, directions, flags, counts -- at HPC, l = 15, density 0.005f, on reads of
200 - 6000 bases (the variant is taken), with mdbg_scan_persistent_info saying which form ran, and with the rows the regions' cursors
handed out (the batch's n_minimizers) equal to the sum of the reads' counts: no read was scanned twice.  "scan_persistent_blocks" caps
the grid so that every wave of a small batch draws many runs.  Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

from metamdbg_amd import synth

pytestmark = pytest.mark.gpu

K = 15
DENSITY = 0.005
BLOCK = 2048                     # positions of a block
LEN_LIMIT = int((176 - 24) / (DENSITY * 0.8 * 1.4))           # 27 142 bases: reads from here on are too long for the variant's stage


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _context(**options):
    from metamdbg_amd import capi
    c = capi.Context(0)
    for name, value in {**dict(scan_prefilter=1, scan_persistent=1, scan_reads_per_wave=0, scan_grab_reads=0), **options}.items():
        c.set_option(name, value)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = _context()
    yield c
    c.close()


def _ascii(codes) -> bytes:
    return bytes(synth.CODE2ASCII[np.asarray(codes, dtype=np.int64)])


def _no_runs(rng, n):
    """n codes, no two neighbours equal: the compressed length is n whatever is stretched afterwards."""
    return np.cumsum(np.concatenate([rng.integers(0, 4, 1), rng.integers(1, 4, n - 1)])) % 4 if n > 1 else rng.integers(0, 4, n)


def _compressed(rng, n) -> bytes:
    """A read whose homopolymer-compressed length is n (its own about 1.75 n)."""
    c = _no_runs(rng, n)
    return _ascii(np.repeat(c, rng.choice([1, 1, 2, 3], len(c))))


@pytest.fixture(scope="module")
def pool():
    """2000 reads of 200 - 6000 bases; the cases take its first n."""
    rng = np.random.default_rng(4242)
    seqs = [_compressed(rng, int(rng.integers(120, 3400))) for _ in range(2000)]
    assert min(len(s) for s in seqs) >= 200 and max(len(s) for s in seqs) <= 6200
    return seqs


_EXPECTED = {}
_EXPECTED_BATCH = {}


def _expected(orc, seqs):
    """The oracle's records of a batch as the arrays a scan hands back; every read's record computed once."""
    key = tuple(id(s) for s in seqs)
    if key not in _EXPECTED_BATCH:
        recs = []
        for s in seqs:
            if s not in _EXPECTED:
                _EXPECTED[s] = orc.read_selection(s, None, K=K, density=DENSITY, hpc=True)
            recs.append(_EXPECTED[s])
        cat = lambda name, dtype: np.concatenate([np.asarray(e[name], dtype=dtype) for e in recs]) if recs else np.zeros(0, dtype)
        _EXPECTED_BATCH[key] = dict(keep=list(seqs), offsets=np.concatenate([[0], np.cumsum([len(e["minimizers"]) for e in recs])]).astype(np.uint64),
                                    minimizers=cat("minimizers", np.uint32), pos=cat("pos", np.uint32), dir=cat("dir", np.uint8),
                                    flags=np.array([1 if e["low_complexity"] else 0 for e in recs], np.uint8))
    return _EXPECTED_BATCH[key]


def _compare(ctx, orc, seqs, form="persistent", launches=1):
    """Scan; every read against readSelection's record; which form ran.  Returns the host arrays."""
    before = ctx.scan_persistent_info()
    reads = ctx.reads_from_ascii(seqs)
    m = ctx.scan(reads, K=K, density=DENSITY, hpc=True, apply_read_filters=True)
    n_rows = m.info()["n_minimizers"]
    h = m.to_host()
    m.free()
    reads.free()
    after = ctx.scan_persistent_info()
    assert after["form"] == form, after
    assert after["persistent_launches"] == before["persistent_launches"] + (launches if form == "persistent" else 0), (before, after)
    if form == "persistent":
        assert after["grab_reads"] >= 1 and after["workgroups"] >= 1
    e = _expected(orc, seqs)
    assert len(h["offsets"]) == len(seqs) + 1
    if not np.array_equal(h["offsets"], e["offsets"]):
        i = int(np.flatnonzero(np.diff(h["offsets"].astype(np.int64)) != np.diff(e["offsets"].astype(np.int64)))[0])
        raise AssertionError(f"read {i} of {len(seqs)} ({len(seqs[i])} bases): {int(h['offsets'][i + 1] - h['offsets'][i])} minimizers, "
                             f"the oracle {int(e['offsets'][i + 1] - e['offsets'][i])}")
    for name in ("minimizers", "pos", "dir"):
        if not np.array_equal(h[name], e[name]):
            row = int(np.flatnonzero(h[name] != e[name])[0])
            raise AssertionError(f"{name}: row {row}, read {int(np.searchsorted(e['offsets'], row, side='right')) - 1} of {len(seqs)}")
    assert np.array_equal(h["flags"], e["flags"])
    # the rows the regions' cursors handed out are the reads' counts (no read is dropped here): none was scanned twice
    assert not e["flags"].any() and n_rows == int(e["offsets"][-1]), (n_rows, int(e["offsets"][-1]))
    return h


# ---- batch sizes around a workgroup's 16 waves, at the default grid -------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, 257, 2000])
def test_batch_sizes_at_the_default_grid(ctx, orc, pool, n):
    h = _compare(ctx, orc, pool[:n])
    info = ctx.scan_persistent_info()
    assert info["grab_reads"] == 4 and info["workgroups"] == -(-n // 64)          # ceil(n / (16 waves x 4)): under one per CU here
    assert int(h["offsets"][-1]) >= 3 * n


# ---- a capped grid: every wave draws many runs; R does not divide n; the last run is partial ------------------------------------
@pytest.mark.parametrize("grab", [1, 2, 3, 8])
@pytest.mark.parametrize("blocks", [1, 2, 3])
@pytest.mark.parametrize("n", [200, 2000])
def test_capped_grids_and_run_lengths(ctx, orc, pool, n, blocks, grab):
    ctx.set_option("scan_persistent_blocks", blocks)
    ctx.set_option("scan_grab_reads", grab)
    try:
        _compare(ctx, orc, pool[:n])
        info = ctx.scan_persistent_info()
        assert info["workgroups"] == min(blocks, -(-n // (16 * grab))) and info["grab_reads"] == grab
    finally:
        ctx.set_option("scan_persistent_blocks", 0)
        ctx.set_option("scan_grab_reads", 0)


# ---- compressed lengths around the block and the tail, mixed in one batch ----------------------------------------------------------
@pytest.mark.parametrize("blocks", [0, 1])
def test_lengths_around_the_block_and_the_tail(ctx, orc, pool, blocks):
    rng = np.random.default_rng(7)
    edge = [_compressed(rng, p + K) for p in (BLOCK - 1, BLOCK, BLOCK + 1)] + [_compressed(rng, 17)]      # 2047 / 2048 / 2049 positions; 30 bases or so
    assert len(edge[3]) <= 40
    seqs = pool[:9] + edge[:2] + pool[9:30] + edge[2:] + pool[30:41] + edge[::-1]
    ctx.set_option("scan_persistent_blocks", blocks)
    try:
        h = _compare(ctx, orc, seqs)
    finally:
        ctx.set_option("scan_persistent_blocks", 0)
    counts = np.diff(h["offsets"].astype(np.int64))
    assert counts[9] >= 1 and counts[10] >= 1 and counts[32] >= 1


# ---- reads the variant passes over: the next item is drawn like after any other --------------------------------------------------
@pytest.mark.parametrize("blocks", [0, 2])
def test_long_reads_are_left_to_the_four_wave_launch(ctx, orc, pool, blocks):
    """Three reads above the variant's length limit among 2000 short ones, holding under 1/32 of the bases: the four-wave kernel scans
    them in a launch of its own and the persistent waves pass over them."""
    rng = np.random.default_rng(31)
    long_ = [_ascii(_no_runs(rng, LEN_LIMIT + 50 * i)) for i in range(3)]
    seqs = pool[:5] + long_[:1] + pool[5:66] + long_[1:2] + pool[66:1999] + long_[2:] + pool[1999:]
    total, over = sum(len(s) for s in seqs), sum(len(s) for s in long_)
    assert over * 32 < total * 3 // 4
    before = ctx.scan_info()
    ctx.set_option("scan_persistent_blocks", blocks)
    try:
        h = _compare(ctx, orc, seqs)
    finally:
        ctx.set_option("scan_persistent_blocks", 0)
    after = ctx.scan_info()
    assert after["block_launches"] == before["block_launches"] + 1 and after["prefiltered_launches"] == before["prefiltered_launches"] + 1
    counts = np.diff(h["offsets"].astype(np.int64))
    assert min(counts[5], counts[67], counts[2001]) >= 60


@pytest.mark.parametrize("blocks", [0, 1])
def test_reads_with_an_n_are_skipped(ctx, orc, pool, blocks):
    """A few reads carry an N: the block kernel leaves them to the general kernel, and its waves go on to the next read."""
    seqs = list(pool[:300])
    for i in (0, 17, 18, 150, 299):
        s = bytearray(seqs[i])
        s[len(s) // 2] = ord("N")
        seqs[i] = bytes(s)
    ctx.set_option("scan_persistent_blocks", blocks)
    try:
        _compare(ctx, orc, seqs)
    finally:
        ctx.set_option("scan_persistent_blocks", 0)


def test_views_go_through_the_persistent_launch(orc, pool):
    """"scan_segments" 2 with segments of 2048 bases: the reads above that are cut into views, scanned by a persistent launch of their own
    (the SEG instantiation) with its own counter; a dead view's wave draws again."""
    c = _context(scan_segments=2, scan_segment_bases=2048, scan_persistent_blocks=2, scan_grab_reads=3)
    try:
        seqs = pool[:400]
        _compare(c, orc, seqs, launches=2)
        cut = c.scan_info()["reads_segmented"]
        assert 0 < cut <= sum(len(s) > 2048 for s in seqs)
        c.set_option("scan_persistent_blocks", 0)
        c.set_option("scan_grab_reads", 0)
        _compare(c, orc, seqs, launches=2)
    finally:
        c.close()


# ---- the counter starts at zero: launch after launch, context beside context --------------------------------------------------------
def test_scans_back_to_back_and_two_contexts_in_turn(ctx, orc, pool):
    other = _context(scan_grab_reads=2)
    try:
        for n in (2000, 257, 33, 2000, 1):
            _compare(ctx, orc, pool[:n])
            _compare(other, orc, pool[:max(1, n // 2)])
        ctx.set_option("scan_persistent_blocks", 1)
        for n in (500, 100, 500):            # one workgroup: a counter left over would leave reads unscanned
            _compare(ctx, orc, pool[:n])
    finally:
        ctx.set_option("scan_persistent_blocks", 0)
        other.close()


# ---- the switch -------------------------------------------------------------------------------------------------------------------
def test_switch_off_and_explicit_reads_per_wave_take_the_chunked_form(ctx, orc, pool):
    seqs = pool[:700]
    persistent = _compare(ctx, orc, seqs)
    try:
        ctx.set_option("scan_persistent", 0)
        chunked = _compare(ctx, orc, seqs, form="chunked")
        ctx.set_option("scan_persistent", 1)
        ctx.set_option("scan_reads_per_wave", 4)
        explicit = _compare(ctx, orc, seqs, form="chunked")
        assert ctx.scan_persistent_info()["workgroups"] == -(-700 // 64) and ctx.scan_persistent_info()["grab_reads"] == 0
    finally:
        ctx.set_option("scan_persistent", 1)
        ctx.set_option("scan_reads_per_wave", 0)
    for name in ("offsets", "minimizers", "pos", "dir", "flags"):
        assert np.array_equal(persistent[name], chunked[name]) and np.array_equal(persistent[name], explicit[name])
    _compare(ctx, orc, seqs)


# ---- a context that shares its device takes the split kernels that fit beside a scan that never retires ---------------------------
def test_a_sharing_context_takes_the_four_wave_split(orc, pool):
    """With "scan_lds_reserve" set and "partition_threads" left at 0, a context whose last scan was a persistent launch takes the four-wave
    split kernels; before its first scan, after a chunked one and with "partition_threads" 512 it takes the eight-wave ones."""
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 60, 500)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    mins = rng.integers(0, 25, int(offs[-1])).astype(np.uint32)
    c = _context(first_pass_mode=2, scan_lds_reserve=28672)
    try:
        forms = []
        for scan_first, persistent, threads in ((False, 1, 0), (True, 1, 0), (True, 0, 0), (True, 1, 512), (True, 1, 256), (True, 1, 0)):
            c.set_option("scan_persistent", persistent)
            c.set_option("partition_threads", threads)
            if scan_first:
                _compare(c, orc, pool[:100], form="persistent" if persistent else "chunked")
                assert c.scan_info()["prefilter_waves"] == 16
            t = c.kminmer_count_first(c.minimizers_from_host(mins, offs), 4, 0)
            assert c.first_pass_info()["path"] == 2 and t.info()["n_records"] > 0
            forms.append(c.first_pass_form())
        small, large = {"split_threads": 256, "split_tile": 1024}, {"split_threads": 512, "split_tile": 4096}
        assert forms == [large, small, large, large, small, small]
    finally:
        c.close()
