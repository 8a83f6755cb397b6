"""What the "kminmer_emit" timer covers in the passes that turn a filled table into rows (csrc/kminmer.hip): the number of intervals
mdbg_timing_get reports for ONE call.  The benchmark reads its per-k kernel milliseconds through these timers, so a launch that moves
into or out of an interval changes what it reports without changing a single result.

  first pass, one table          2   slot_flag_kernel | emit_slots_kernel + emit_rescued_kernel
  refined pass, slots            2   (refine_slots_kernel +) slot_flag_kernel | emit_slots_kernel
  refined pass, buckets          2   bucket_flag_kernel | bucket_emit_kernel
  index pass, slots              1   emit_slots_kernel (its slot_flag_kernel is untimed)
  index pass, buckets            2   bucket_flag_kernel | bucket_emit_kernel

GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 5


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    c.timing(True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reads(ctx):
    """A few hundred reads over a genome of distinct minimizers, either orientation, a quarter of them with one error."""
    rng = np.random.default_rng(305)
    genome = rng.permutation(5000).astype(np.uint32)
    rl = []
    for _ in range(600):
        a = int(rng.integers(0, 4900)); n = int(rng.integers(0, 80))
        seg = genome[a:a + n]
        if rng.integers(0, 2): seg = seg[::-1]
        seg = seg.copy()
        if n and rng.integers(0, 4) == 0: seg[int(rng.integers(0, n))] = 6000 + int(rng.integers(0, 50))
        rl.append(seg)
    offs = np.concatenate([[0], np.cumsum([len(x) for x in rl])]).astype(np.uint64)
    return ctx.minimizers_from_host(np.concatenate(rl).astype(np.uint32), offs)


@pytest.fixture(scope="module")
def prev(ctx, reads):
    ctx.set_option("first_pass_mode", 1)
    try:
        return ctx.kminmer_count_first(reads, K - 1, 0)
    finally:
        ctx.set_option("first_pass_mode", 0)


def _emit_intervals(ctx, call):
    ctx.timing_reset()
    t = call()
    n = ctx.timing_get("kminmer_emit")[1]
    print(f"kminmer_emit intervals: {n}")
    return t, n


def test_first_pass_one_table(ctx, reads):
    ctx.set_option("first_pass_mode", 1)
    try:
        t, n = _emit_intervals(ctx, lambda: ctx.kminmer_count_first(reads, K - 1, 0))
    finally:
        ctx.set_option("first_pass_mode", 0)
    info = t.info()
    assert info["n_records"] > info["n_solid"] > 0, "the input is meant to have rescued rows"
    assert n == 2


@pytest.mark.parametrize("form,expected", [("slots", 2), ("buckets", 2)])
def test_refined_pass(ctx, reads, prev, form, expected):
    ctx.set_option("refined_form", 0 if form == "buckets" else 1)
    ctx.set_option("index_table_form", 0 if form == "buckets" else 1)
    try:
        t, n = _emit_intervals(ctx, lambda: ctx.kminmer_count_refined(reads, None, K, prev))
    finally:
        ctx.set_option("refined_form", 1)
        ctx.set_option("index_table_form", 1)
    assert t.info()["n_records"] > 0
    assert n == expected


@pytest.mark.parametrize("form,expected", [("slots", 1), ("buckets", 2)])
def test_index_pass(ctx, reads, prev, form, expected):
    ctx.set_option("index_table_form", 0 if form == "buckets" else 1)
    try:
        t, n = _emit_intervals(ctx, lambda: ctx.kminmer_index(reads, None, K, prev))
    finally:
        ctx.set_option("index_table_form", 1)
    assert t.info()["n_records"] > 0
    assert n == expected
