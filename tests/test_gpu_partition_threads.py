"""The two forms of the radix split's kernels (csrc/partition.hip, "partition_threads"): four waves a block and tiles of 1024 records --
what fits beside another context's 16-wave scan workgroup by registers, DESIGN.md 4.4 -- against eight waves and tiles of 2048 / 4096, and
both against the oracle's table.  k = 4; the multiset of (key, abundance) and n_solid must agree exactly.  The batches sit around the small
form's tile (1023 / 1024 / 1025 instances, 2 tiles + 1) where a wrong tile bound or a dropped partial tile loses records, plus one of
about 100 000 minimizers that gives every block several tiles.  GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

from metamdbg_amd import formats

pytestmark = pytest.mark.gpu

K = 4
SMALL_THREADS, SMALL_TILE = 256, 1024
# the options bench.py gives every context that shares its device (its shared_opts)
BENCH_SHARED = {"scan_lds_reserve": 28672, "partition_tile": 2048, "partition_slot_list": 0, "partition_lds_slots": 1024}
OPTION_NAMES = ("first_pass_mode", "partition_bits", "partition_lds_slots", "partition_max_records", "partition_threads", "partition_tile",
                "scan_lds_reserve")
# one split level, two, three (the plans of tests/test_gpu_partition.py), several groups of keys
PLANS = [dict(), dict(partition_bits=3), dict(partition_bits=10), dict(partition_bits=17, partition_lds_slots=256), dict(partition_max_records=1500),
         dict(partition_max_records=300, partition_bits=9)]


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


def _set(ctx, **kw):
    for name in OPTION_NAMES:
        ctx.set_option(name, kw.get(name, 0))
    ctx.set_option("partition_slot_list", kw.get("partition_slot_list", 1))


def _batch(seed, n_instances, alphabet, one_read=False):
    """Reads in minimizer space with exactly n_instances windows of K; empty reads and reads shorter than K are among them.  Every
    second read repeats ONE minimizer: about half of the instances are one (palindromic) key, so below level 1 -- where a block's share
    is otherwise a single tile at these sizes -- one segment is many tiles long and one block walks them all."""
    rng = np.random.default_rng(seed)
    if one_read:
        lens = [n_instances + K - 1]
    else:
        lens, left = [], n_instances
        while left > 0:
            n = int(rng.integers(0, 60))
            inst = max(n - (K - 1), 0)
            if inst > left:
                n, inst = left + K - 1, left
            lens.append(n)
            left -= inst
        lens += [0, 2, K - 1]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    mins = rng.integers(0, alphabet, int(offs[-1])).astype(np.uint32)
    for r in range(0, len(lens), 2):
        mins[int(offs[r]): int(offs[r + 1])] = 3
    assert int(np.maximum(np.diff(offs.astype(np.int64)) - (K - 1), 0).sum()) == n_instances
    return mins, offs


# name -> (instances, alphabet, one read): small alphabets make most keys solid
BATCHES = {
    "tile-1": (SMALL_TILE - 1, 6, False), "tile": (SMALL_TILE, 6, False), "tile+1": (SMALL_TILE + 1, 6, False),
    "2tiles+1": (2 * SMALL_TILE + 1, 6, False), "one-read-tile+1": (SMALL_TILE + 1, 6, True), "100k": (96_000, 14, False),
}
_cache: dict = {}


def _reference(orc, name):
    """The batch and the oracle's table of it: made once, shared by every case, never written to."""
    if name not in _cache:
        n, alphabet, one = BATCHES[name]
        mins, offs = _batch(40 + len(_cache), n, alphabet, one)
        exp = orc.kminmer_count_first(mins, offs, K, 0)
        want = formats.sorted_abundance_records(orc.table_abundance_records(exp))
        for a in (mins, offs, want):
            a.setflags(write=False)
        _cache[name] = (mins, offs, exp["n_solid"], want)
    return _cache[name]


def _count(ctx, mins, offs, **options):
    _set(ctx, **options)
    try:
        t = ctx.kminmer_count_first(ctx.minimizers_from_host(mins, offs), K, 0)
        info, form = ctx.first_pass_info(), ctx.first_pass_form()
    finally:
        _set(ctx)
    rec, _ = t.to_host()
    return formats.sorted_abundance_records(rec), t.info()["n_solid"], info, form


@pytest.mark.parametrize("plan", range(len(PLANS)))
@pytest.mark.parametrize("batch", list(BATCHES))
def test_split_forms_agree_with_each_other_and_the_oracle(ctx, orc, batch, plan):
    mins, offs, n_solid, want = _reference(orc, batch)
    got = {}
    for threads in (256, 512):
        rec, ns, info, form = _count(ctx, mins, offs, first_pass_mode=2, partition_threads=threads, **PLANS[plan])
        assert info["path"] == 2 and info["instances"] == BATCHES[batch][0], info
        assert form["split_threads"] == threads, form
        assert form["split_tile"] == (SMALL_TILE if threads == 256 else 4096), form
        if PLANS[plan].get("partition_max_records", 1 << 40) < BATCHES[batch][0]:
            assert info["groups"] > 1, info
        if PLANS[plan].get("partition_bits", 0) > 8:
            assert info["levels"] == (PLANS[plan]["partition_bits"] + 7) // 8, info
        got[threads] = (rec, ns)
    for threads, (rec, ns) in got.items():
        assert ns == n_solid, (threads, ns, n_solid)
        assert np.array_equal(rec, want), threads
    assert np.array_equal(got[256][0], got[512][0]) and got[256][1] == got[512][1]


def test_form_a_device_sharing_context_takes(ctx, orc):
    """bench.py's shared options.  The four-wave forms were built to be what such a context takes by itself; measured beside the
    16-wave scan they are slower than the eight-wave ones and the scan no faster (1166.8 - 1178.4 against
    1181.0 - 1184.8 Gbp/s, three alternating runs each), so the automatic choice stays with eight waves and the small tile, and
    "partition_threads" 256 is what selects the four-wave forms -- for such a context too."""
    mins, offs, n_solid, want = _reference(orc, "100k")
    rec, ns, info, form = _count(ctx, mins, offs, first_pass_mode=2, **BENCH_SHARED)
    assert info["path"] == 2 and info["lds_slots"] == 1024, info
    assert form == {"split_threads": 512, "split_tile": 2048}, form
    assert ns == n_solid and np.array_equal(rec, want)
    rec, ns, info, form = _count(ctx, mins, offs, first_pass_mode=2, partition_threads=256, **BENCH_SHARED)
    assert info["path"] == 2 and info["lds_slots"] == 1024, info
    assert form == {"split_threads": SMALL_THREADS, "split_tile": SMALL_TILE}, form
    assert ns == n_solid and np.array_equal(rec, want)


@pytest.mark.parametrize("threads", [256, 512])
def test_short_reads_and_empty_batch(ctx, orc, threads):
    """No read has a window (but the batch has K minimizers: the partitioned pass takes it); then a batch of no reads at all."""
    lens = [0, 1, 2, 3, 3, 0, 2, 1, 3]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    mins = np.arange(int(offs[-1]), dtype=np.uint32) % 5
    rec, ns, info, form = _count(ctx, mins, offs, first_pass_mode=2, partition_threads=threads)
    assert info["path"] == 2 and info["instances"] == 0 and form["split_threads"] == threads, (info, form)
    assert len(rec) == 0 and ns == 0
    # short reads among others: only the one long read counts
    lens = [3, 0, 9, 2]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    mins = np.array([1, 2, 3, 7, 8, 9, 7, 8, 9, 7, 8, 9, 4, 4], dtype=np.uint32)
    exp = orc.kminmer_count_first(mins, offs, K, 0)
    rec, ns, info, _ = _count(ctx, mins, offs, first_pass_mode=2, partition_threads=threads)
    assert info["instances"] == 6 and ns == exp["n_solid"]
    assert np.array_equal(rec, formats.sorted_abundance_records(orc.table_abundance_records(exp)))
    rec, ns, info, _ = _count(ctx, np.zeros(0, np.uint32), np.zeros(1, np.uint64), first_pass_mode=2, partition_threads=threads)
    assert len(rec) == 0 and ns == 0


def test_partition_threads_rejects_other_values(ctx):
    from metamdbg_amd import capi
    with pytest.raises(capi.MdbgError):
        ctx.set_option("partition_threads", 128)
    _set(ctx)
