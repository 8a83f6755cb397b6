"""sort_u64_pairs (csrc/prims.hip: sort_bits_kernel, sort_hist_kernel, sort_scatter_kernel) called directly through
mdbg_bytes_sort_u64_pairs: a stable least-significant-digit radix sort of 64-bit keys with a 32-bit value, eight bits a pass.  Every
result is compared for equality with numpy.argsort(kind="stable") -- keys and values, so equal keys must keep their value order.

Geometry the sizes are cut to: a block owns a tile of 4096 items, a wave 1024 of them in 16 rounds of 64; the last tile's missing items
are idle lanes of its last rounds.  A digit in which all keys agree is skipped, so the number of passes that ran is part of the result.
The bytes behind the last key and the last value are a pattern that must survive.

Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 4096
SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 5 * TILE + 777, 1 << 20]
GUARD = 32


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def keys_of(pattern: str, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if pattern == "equal":
        return np.full(n, 0x0123456789ABCDEF, np.uint64)
    if pattern == "top_byte":
        return (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56)) | np.uint64(0x00AAAAAAAAAAAAAA)
    if pattern == "bottom_byte":
        return rng.integers(0, 256, n, dtype=np.uint64) | np.uint64(0x5555555555555500)
    if pattern == "random":
        return rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if pattern == "few_distinct":           # long runs of equal keys in every digit that differs: stability is most of the result
        return rng.integers(0, 5, n, dtype=np.uint64) * np.uint64(0x0001000100010001)
    if pattern == "mapper":                 # (query << 32 | window): two dense 32-bit halves, as mdbg_map_anchors sorts them
        return (rng.integers(0, 300, n, dtype=np.uint64) << np.uint64(32)) | rng.integers(0, 5000, n, dtype=np.uint64)
    raise ValueError(pattern)


def sort_on_device(ctx, keys: np.ndarray, values: np.ndarray) -> tuple:
    n = len(keys)
    kb = ctx.bytes_from_host(keys.tobytes() + bytes([0xC3]) * GUARD)
    vb = ctx.bytes_from_host(values.tobytes() + bytes([0x3C]) * GUARD)
    info = ctx.bytes_sort_u64_pairs(kb, 0, vb, 0, n)
    k = np.frombuffer(kb.download(0, 8 * n + GUARD), np.uint8)
    v = np.frombuffer(vb.download(0, 4 * n + GUARD), np.uint8)
    assert (k[8 * n:] == 0xC3).all() and (v[4 * n:] == 0x3C).all(), "bytes behind the last item were written"
    kb.free(); vb.free()
    return k[:8 * n].view(np.uint64), v[:4 * n].view(np.uint32), info


def check(ctx, keys: np.ndarray, values: np.ndarray) -> dict:
    k, v, info = sort_on_device(ctx, keys, values)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(k, keys[order])
    assert np.array_equal(v, values[order]), "equal keys did not keep their order"
    differ = np.bitwise_or.reduce(keys) ^ np.bitwise_and.reduce(keys) if len(keys) > 1 else np.uint64(0)
    live = sum(1 for d in range(8) if (int(differ) >> (8 * d)) & 255)
    assert info == dict(passes_run=live, passes_skipped=8 - live), (info, live)
    return info


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", ["equal", "top_byte", "bottom_byte", "random"])
def test_sizes_and_key_patterns(ctx, pattern, n):
    keys = keys_of(pattern, n, 1000 + n)
    info = check(ctx, keys, np.arange(n, dtype=np.uint32))
    if n > 300:
        assert info["passes_run"] == dict(equal=0, top_byte=1, bottom_byte=1, random=8)[pattern]


@pytest.mark.parametrize("pattern", ["few_distinct", "mapper"])
@pytest.mark.parametrize("n", [TILE + 1, 9 * TILE + 5])
def test_stability_with_values_that_are_no_ranks(ctx, pattern, n):
    """Values in no relation to the input order: a sort that ordered equal keys by value instead of by position would show."""
    rng = np.random.default_rng(n)
    check(ctx, keys_of(pattern, n, n), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))


def test_ranges_inside_one_buffer_and_refusals(ctx):
    from metamdbg_amd import capi
    n = 3000
    keys = keys_of("random", n, 5)
    vals = np.arange(n, dtype=np.uint32)[::-1].copy()
    raw = bytes(16) + keys.tobytes() + bytes(8) + vals.tobytes() + bytes(4)
    b = ctx.bytes_from_host(raw)
    ctx.bytes_sort_u64_pairs(b, 16, b, 16 + 8 * n + 8, n)
    out = np.frombuffer(b.download(0, len(raw)), np.uint8)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(out[16:16 + 8 * n].view(np.uint64), keys[order]) and np.array_equal(out[24 + 8 * n:24 + 12 * n].view(np.uint32), vals[order])
    assert not out[:16].any() and not out[16 + 8 * n:24 + 8 * n].any() and not out[24 + 12 * n:].any()
    for args in ((b, 4, b, 16 + 8 * n + 8, n), (b, 16, b, 16 + 8 * n + 6, n), (b, 16, b, 16 + 8 * n + 8, n + 2), (b, 16, b, 16 + 8 * n - 4, n), (None, 0, b, 0, 1), (b, 0, None, 0, 1)):
        with pytest.raises(capi.MdbgError) as e:
            ctx.bytes_sort_u64_pairs(*args)
        assert e.value.code == -1
    b.free()


def test_timer_and_kernel_attributes(ctx):
    ctx.timing(True)
    ctx.timing_reset()
    try:
        check(ctx, keys_of("random", 3 * TILE, 9), np.arange(3 * TILE, dtype=np.uint32))
        ctx.synchronize()
        ms, launches = ctx.timing_get("radix_sort")
    finally:
        ctx.timing(False)
    assert launches == 1 and ms > 0
    for name in ("sort_bits", "sort_bits_fold", "sort_hist", "sort_scatter"):
        a = ctx.kernel_attributes(name)
        assert a["scratch"] == 0 and 0 < a["registers"] <= 64, (name, a)
    assert ctx.kernel_attributes("sort_scatter")["static_lds"] == 4096 and ctx.kernel_attributes("sort_hist")["static_lds"] == 1024
