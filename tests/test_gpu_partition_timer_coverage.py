"""What the launch timers cover in the partitioned first pass and its sharded halves (csrc/partition.hip): the number of intervals
mdbg_timing_get reports for ONE call under each of "kminmer_split", "kminmer_insert", "kminmer_rescue", "kminmer_emit", "shard_rows" and
"shard_reduce".  The benchmark reads its per-kernel milliseconds through these timers, so a LaunchTimer object that appears, disappears
or swallows a prefix scan changes what it reports, and the event traffic of a step, without changing a single result.

The inputs are those of tests/test_gpu_partition.py (400 random minimizer reads, k = 4, "first_pass_mode" 2), the plan forced by
"partition_bits" so that the sketch does not decide the shape -- but for one call, in a context of its own, which the sketch plans.
How the numbers read: per call, mark_starts is one "kminmer_split" object; per attempt and key group, level 1 is two (histogram,
scatter; three when the sketch runs, whose histogram is repeated for an input this small) and every deeper level two more; the bucket
count is one "kminmer_insert" per attempt and group; the rescue count one "kminmer_rescue" per attempt at one group (min_abundance <= 1;
the overflow is only read with its total), one per call with key groups; the rows one "kminmer_emit" per group kept aside plus one for the
table.  They were recorded from the library as it stood before the host half of partition.hip was rewritten
(profiles/partition_timer_coverage_parent.txt) and are not to follow the code.

The owner's bucket form is pinned by tests/test_gpu_shard_chosen_keys.py (2^17 rows, one "shard_reduce" entry); the exchange here is the
one-table form's.  GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

from tests.test_gpu_partition import _options, _random_minimizer_reads

pytestmark = pytest.mark.gpu

K = 4
TIMERS = ("kminmer_split", "kminmer_insert", "kminmer_rescue", "kminmer_emit", "shard_rows", "shard_reduce")

# name -> (options, what first_pass_info must say of the call)
PLANS = {
    "one_level": (dict(partition_bits=3), dict(levels=1, groups=1)),
    "two_levels": (dict(partition_bits=10), dict(levels=2, attempts=1, groups=1)),
    "three_levels": (dict(partition_bits=17, partition_lds_slots=256), dict(levels=3, attempts=1, groups=1)),
    "overflow_repeat": (dict(partition_bits=3, partition_lds_slots=256), dict(groups=1)),
    "key_groups": (dict(partition_max_records=300, partition_bits=9), dict(attempts=1)),
}

# (split, insert, rescue, emit, shard_rows, shard_reduce) of one mdbg_kminmer_count_first, by plan and min_abundance
EXPECTED_FIRST = {
    ("one_level", 0): (5, 2, 2, 1, 0, 0), ("one_level", 2): (5, 2, 0, 1, 0, 0),                  # (8 x 1024 slots overflow once: two attempts)
    ("two_levels", 0): (5, 1, 1, 1, 0, 0), ("two_levels", 2): (5, 1, 0, 1, 0, 0),
    ("three_levels", 0): (7, 1, 1, 1, 0, 0), ("three_levels", 2): (7, 1, 0, 1, 0, 0),
    ("overflow_repeat", 0): (7, 3, 3, 1, 0, 0), ("overflow_repeat", 2): (7, 3, 0, 1, 0, 0),      # three attempts
    ("key_groups", 0): (257, 64, 1, 65, 0, 0), ("key_groups", 2): (257, 64, 0, 65, 0, 0),        # 64 groups
}
# ... of mdbg_shard_begin, mdbg_shard_exchange_local and mdbg_shard_finish on one partitioned share ("partition_bits" 3), by min_abundance
EXPECTED_SHARD = {
    0: dict(begin=(5, 2, 0, 0, 3, 0), exchange=(0, 0, 0, 0, 0, 2), finish=(0, 1, 1, 1, 0, 0)),
    2: dict(begin=(5, 2, 0, 0, 3, 0), exchange=(0, 0, 0, 0, 0, 2), finish=(0, 0, 0, 1, 0, 0)),
}
# ... of one unforced mdbg_kminmer_count_first in a fresh context, by min_abundance
EXPECTED_UNFORCED = {0: (4, 1, 1, 1, 0, 0), 2: (4, 1, 0, 1, 0, 0)}


def _mins():
    rng = np.random.default_rng(1000 + 17 * K)
    return _random_minimizer_reads(rng, 400, 25)


def _new_ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    c.timing(True)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = _new_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def reads(ctx):
    return ctx.minimizers_from_host(*_mins())


def _intervals(ctx, call):
    ctx.timing_reset()
    out = call()
    return out, tuple(int(ctx.timing_get(name)[1]) for name in TIMERS)


def measure_first(ctx, reads, options, min_ab):
    """One mdbg_kminmer_count_first under `options`: (first_pass_info, intervals per timer)."""
    _options(ctx, first_pass_mode=2, **options)
    try:
        _, n = _intervals(ctx, lambda: ctx.kminmer_count_first(reads, K, min_ab))
        return ctx.first_pass_info(), n
    finally:
        _options(ctx)


def measure_shard(ctx, reads, min_ab):
    """The three calls of a sharded first pass of one rank whose share the partitioned pass takes: intervals per timer of each."""
    from metamdbg_amd import capi
    _options(ctx, first_pass_mode=2, partition_bits=3)
    try:
        sh, begin = _intervals(ctx, lambda: ctx.shard_begin(reads, K, 1))
        info = ctx.first_pass_info()
        replies, exchange = _intervals(ctx, lambda: capi.exchange_local(ctx, [sh]))
        _, finish = _intervals(ctx, lambda: sh.finish(replies[0], min_ab))
        return info, dict(begin=begin, exchange=exchange, finish=finish)
    finally:
        _options(ctx)


def measure_unforced(min_ab):
    """A context of its own: the key-ratio hint that sizes level 1 before the sketch is the initial one."""
    c = _new_ctx()
    try:
        return measure_first(c, c.minimizers_from_host(*_mins()), dict(), min_ab)
    finally:
        c.close()


@pytest.mark.parametrize("min_ab", [0, 2])
@pytest.mark.parametrize("plan", list(PLANS))
def test_count_first_intervals(ctx, reads, plan, min_ab):
    options, shape = PLANS[plan]
    info, n = measure_first(ctx, reads, options, min_ab)
    print(f"{plan} min_abundance {min_ab}: {dict(zip(TIMERS, n))} {info}")
    assert info["path"] == 2, info
    for key, value in shape.items():
        assert info[key] == value, info
    if plan == "overflow_repeat":
        assert info["attempts"] > 1, info
    if plan == "key_groups":
        assert info["groups"] > 1, info
    assert n == EXPECTED_FIRST[plan, min_ab]


@pytest.mark.parametrize("min_ab", [0, 2])
def test_sharded_share_intervals(ctx, reads, min_ab):
    info, n = measure_shard(ctx, reads, min_ab)
    print(f"shard min_abundance {min_ab}: {n} {info}")
    assert info["path"] == 2 and info["levels"] == 1, info
    assert n == EXPECTED_SHARD[min_ab]


@pytest.mark.parametrize("min_ab", [0, 2])
def test_unforced_call_intervals(min_ab):
    info, n = measure_unforced(min_ab)
    print(f"unforced min_abundance {min_ab}: {dict(zip(TIMERS, n))} {info}")
    assert info["path"] == 2, info
    assert n == EXPECTED_UNFORCED[min_ab]
