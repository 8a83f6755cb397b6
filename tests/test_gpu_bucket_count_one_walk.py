"""bucket_count's one walk over the keys (csrc/partition.hip): the form without a slot list keeps the LDS slot of a thread's first 16
records -- four trips of four, 8192 records a bucket -- in registers between its two walks, so the second walk loads only `rep`; the
records behind them (with a slot list: those behind the list) find their slot again by their key, which first_pass_slot_fall_backs()
counts.  k = 4 against the oracle: the whole record multiset -- rescued rows included -- and n_solid must agree exactly.

The batch is ONE bucket (few enough keys for no bucket bits beside 2048 slots) of reads of five minimizers, two instances each, so an
instance's place in the bucket is its place in the batch up to the scatter's tile (1024 positions, about 410 instances, regrouped in
LDS).  Most reads repeat one minimizer: a key counted far above the clip, whose byte is the default 0 and is never stored.  The RARE
reads come in pairs [u, s1 .. s4], [u', s1 .. s4]: one window seen once, one seen twice, so both reads are rescued and the count-1
windows become rows only if their byte says 1 -- a dropped slot leaves 0 (the row is missing), a neighbour's slot says 2 or 0 (missing)
or gives a count-2 window a 1 (a row too many).  Rare reads sit in the middle of each of the four kept trips (instances 2048 t + 700 ..
+ 900) and fill everything from instance 7400 on, so with exactly 8192 instances the last record of the last kept trip, whichever
thread holds it, is rare; and there are under 1300 distinct keys, which one table of 2048 slots takes.  GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

from metamdbg_amd import formats

pytestmark = pytest.mark.gpu

K = 4
TRIP = 4 * 512                      # records of a bucket per trip (BC_U * BC_NT)
KEPT = 4 * TRIP                     # ... whose slot is kept in registers (BC_KEEP_TRIPS trips)
OPTION_NAMES = ("first_pass_mode", "partition_lds_slots", "partition_threads")


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


def _rare_instance(i):
    return any(TRIP * t + 700 <= i < TRIP * t + 900 for t in range(4)) or i >= 7400


def _batch(n_reads, extra_front):
    """n_reads reads of five minimizers (instances 2 r and 2 r + 1), rare where _rare_instance says; extra_front frequent reads first."""
    rng = np.random.default_rng(9)
    rare = [r for r in range(n_reads) if _rare_instance(2 * r)]
    if len(rare) % 2:
        rare = rare[1:]
    fresh = iter(rng.permutation(np.arange(1000, 200000, dtype=np.uint32)))
    mins = np.full((n_reads, 5), 3, dtype=np.uint32)
    for a, b in zip(rare[0::2], rare[1::2]):
        shared = [next(fresh) for _ in range(4)]
        mins[a] = [next(fresh)] + shared
        mins[b] = [next(fresh)] + shared
    mins = np.concatenate([np.full((extra_front, 5), 3, dtype=np.uint32), mins]).reshape(-1)
    offs = (np.arange(n_reads + extra_front + 1, dtype=np.uint64) * 5)
    return mins, offs, len(rare)


_cache: dict = {}


def _reference(orc, name):
    """The batch and the oracle's table of it: made once, shared by the cases, never written to."""
    if name not in _cache:
        mins, offs, n_rare = _batch(KEPT // 2, {"exact": 0, "one-read-more": 1}[name])
        exp = orc.kminmer_count_first(mins, offs, K, 0)
        want = formats.sorted_abundance_records(orc.table_abundance_records(exp))
        for a in (mins, offs, want):
            a.setflags(write=False)
        _cache[name] = (mins, offs, n_rare, exp["n_solid"], want)
    return _cache[name]


def _count(ctx, mins, offs, **options):
    _set(ctx, **options)
    try:
        t = ctx.kminmer_count_first(ctx.minimizers_from_host(mins, offs), K, 0)
        info, fell_back = ctx.first_pass_info(), ctx.first_pass_slot_fall_backs()
    finally:
        _set(ctx)
    rec, _ = t.to_host()
    return formats.sorted_abundance_records(rec), t.info(), info, fell_back


@pytest.mark.parametrize("slot_list", [0, 1])
@pytest.mark.parametrize("name", ["exact", "one-read-more"])
def test_one_walk_against_the_oracle(ctx, orc, name, slot_list):
    mins, offs, n_rare, n_solid, want = _reference(orc, name)
    # what the batch is built to be: every rare read rescued, a row for its count-1 window and one per pair for the shared one
    assert n_rare >= 4 * 98 + 394 and 3 * (n_rare // 2) < 1300 and n_solid == n_rare // 2 + 1 and len(want) == n_solid + n_rare, (n_rare, n_solid, len(want))
    rec, tinfo, info, fell_back = _count(ctx, mins, offs, first_pass_mode=2, partition_lds_slots=2048, partition_threads=256, partition_slot_list=slot_list)
    n = KEPT + (2 if name == "one-read-more" else 0)
    assert info["path"] == 2 and info["buckets"] == 1 and info["attempts"] == 1 and info["instances"] == n, info
    print(name, slot_list, tinfo, "fall-backs", fell_back)
    assert fell_back == (n - 4096 if slot_list else n - KEPT), fell_back        # (the list beside 2048 slots holds 4096)
    assert tinfo["n_solid"] == n_solid, (tinfo, n_solid)
    assert tinfo["n_records"] == len(want) and np.array_equal(rec, want)
