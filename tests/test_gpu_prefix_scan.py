"""The device-wide exclusive prefix sum (csrc/prims.hip: scan_reduce_kernel, scan_small_kernel, scan_apply_kernel, exclusive_scan_impl)
called directly through mdbg_bytes_prefix_sum on chosen sizes, values and alignments, every one of the n + 1 sums compared for equality
with numpy's cumulative sum in uint64.

Geometry the cases are cut to: a block owns 4096 items in 4 sub-tiles of 256 threads x 4 items; a lane's 4 items are one vector load
when they lie inside n and their address is 16-byte (u32) / 32-byte (u64) aligned and four guarded loads otherwise; the sums of a whole
quad leave as two 16-byte stores when `out` is 16-byte aligned and as four 8-byte stores otherwise, those of the quad that straddles n one
by one.  More than "prefix_small_limit" block sums (65536: above 2^28 items) are scanned by the same kernels recursively, copied back and
waited for; the option brings that to a few thousand items.

Alignment of an mdbg_bytes: mdbg_bytes_create takes a whole block of the context's pool (DevPool::get), which hands out hipMalloc
blocks in size classes of at least 256 bytes and never cuts one up; hipMalloc aligns to 256 bytes or more.  So byte 0 of a buffer is
at least 32-byte aligned, and byte offset `at` has the alignment of `at` itself: in_at 0 takes the vector loads, in_at 4 / 8 / 12 (u32)
and 8 / 16 / 24 (u64) the guarded ones; out_at 0 the 16-byte stores, out_at 8 the 8-byte ones.

Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 4096
SEAMS = [0, 1, 2, 3, 4, 5, 255, 256, 257, 1020, 1023, 1024, 1025, 4092, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 1021]
DTYPE = {4: np.dtype("<u4"), 8: np.dtype("<u8")}
PATTERN = 0xA5
TAIL = 24                                   # pattern bytes kept behind the last sum (and behind the last input value)


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def reference(v) -> np.ndarray:
    """[0, v0, v0 + v1, ...] in uint64 (the zero is a uint64 too: a Python 0 in front would make numpy promote the whole array to float64)."""
    return np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(np.asarray(v).astype(np.uint64), dtype=np.uint64)])


def random_values(width: int, n: int, seed: int) -> np.ndarray:
    """u32: the full range, so that the sums pass 2^32 from the third item on; u64: below 2^52, so that no sum of the sizes here wraps."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2**32 if width == 4 else 2**52, n, dtype=np.uint64).astype(DTYPE[width])


class Job:
    """One scan in three steps: the input and a pattern-filled output uploaded (the host waits for both copies), the scan queued
    (`launch`: nothing but the library's call, no wait), the output checked whole -- guards included -- when asked (`sums`)."""

    def __init__(self, ctx, v: np.ndarray, in_at: int = 0, out_at: int = 0):
        self.ctx, self.v, self.in_at, self.out_at = ctx, v, in_at, out_at
        self.width, self.n = v.dtype.itemsize, len(v)
        self.raw_in = bytes([PATTERN]) * in_at + v.tobytes() + bytes([PATTERN]) * TAIL
        self.n_out = out_at + 8 * (self.n + 1) + TAIL
        self.d_in = self.d_out = None
        try:
            self.d_in = ctx.bytes_from_host(self.raw_in)
            self.d_out = ctx.bytes_from_host(bytes([PATTERN]) * self.n_out)
        except BaseException:
            self.free()
            raise

    def launch(self) -> "Job":
        self.ctx.bytes_prefix_sum(self.d_in, self.in_at, self.width, self.n, self.d_out, self.out_at)
        return self

    def sums(self) -> np.ndarray:
        """The n + 1 sums, after the bytes in front of and behind them and the whole input were found untouched."""
        raw = self.d_out.download(0, self.n_out)
        end = self.out_at + 8 * (self.n + 1)
        assert raw[:self.out_at] == bytes([PATTERN]) * self.out_at, "bytes in front of out_at were written"
        assert raw[end:] == bytes([PATTERN]) * TAIL, "bytes behind the total were written"
        assert self.d_in.download(0, len(self.raw_in)) == self.raw_in, "the input changed"
        return np.frombuffer(raw[self.out_at:end], dtype="<u8")

    def free(self):
        for b in (self.d_in, self.d_out):
            if b is not None:
                b.free()
        self.d_in = self.d_out = None


def scan(ctx, v, in_at: int = 0, out_at: int = 0) -> np.ndarray:
    job = Job(ctx, v, in_at, out_at)
    try:
        return job.launch().sums()
    finally:
        job.free()


def same(got: np.ndarray, exp: np.ndarray, what=""):
    assert got.dtype == np.uint64 and exp.dtype == np.uint64 and got.shape == exp.shape, what
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{what}: {bad.size} of {len(exp)} sums differ, the first at {int(bad[0])}: {int(got[bad[0]])} for {int(exp[bad[0]])}"


class limit:
    """"prefix_small_limit" for a block of code, the default again behind it."""

    def __init__(self, ctx, value):
        self.ctx, self.value = ctx, value

    def __enter__(self):
        self.ctx.set_option("prefix_small_limit", self.value)

    def __exit__(self, *exc):
        self.ctx.set_option("prefix_small_limit", 0)
        return False


# ---- sizes at every seam -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SEAMS)
@pytest.mark.parametrize("width", [4, 8])
def test_sizes_at_every_seam(ctx, width, n):
    v = random_values(width, n, seed=1000 * width + n)
    exp = reference(v)
    if width == 4 and n >= 16:
        assert int(exp[16]) >= 2**32                            # (full-range values: the sums leave 32 bits within the first lanes' items)
    same(scan(ctx, v), exp, (width, n))


# ---- extreme values ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4097, 8193])
def test_every_item_all_ones(ctx, n):
    got = scan(ctx, np.full(n, 0xFFFFFFFF, dtype="<u4"))
    assert int(got[n]) == n * (2**32 - 1)
    same(got, np.arange(n + 1, dtype=np.uint64) * np.uint64(2**32 - 1), n)
    same(got, reference(np.full(n, 0xFFFFFFFF, dtype="<u4")), n)


@pytest.mark.parametrize("n", [4097, 8193])
@pytest.mark.parametrize("width", [4, 8])
def test_every_item_zero(ctx, width, n):
    same(scan(ctx, np.zeros(n, dtype=DTYPE[width])), np.zeros(n + 1, dtype=np.uint64), (width, n))


# ---- one non-zero item: each carry by itself ---------------------------------------------------------------------------------------------
N_ONE = 2 * TILE + 7


@pytest.mark.parametrize("p", [0, 3, 4, 255, 256, 1023, 1024, 4095, 4096, 4097, N_ONE - 1])
@pytest.mark.parametrize("width", [4, 8])
def test_one_non_zero_item(ctx, width, p):
    """0 up to and including p, 1 behind it: lane to wave (3 | 4, 255 | 256), wave to block and sub-tile to sub-tile (1023 | 1024), block to
    block (4095 | 4096), and the total alone (n - 1)."""
    v = np.zeros(N_ONE, dtype=DTYPE[width])
    v[p] = 1
    exp = (np.arange(N_ONE + 1) > p).astype(np.uint64)
    same(exp, reference(v))
    same(scan(ctx, v), exp, (width, p))


# ---- alignment and guards ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4095, 4097])
@pytest.mark.parametrize("out_at", [0, 8])
@pytest.mark.parametrize("width,in_at", [(4, 0), (4, 4), (4, 8), (4, 12), (8, 0), (8, 8), (8, 16), (8, 24)])
def test_alignment_and_guards(ctx, width, in_at, out_at, n):
    """Both load paths (in_at 0 against the others) and both store paths (out_at 0 against 8), see the module's text; `scan` checks the
    pattern bytes in front of out_at and behind out_at + 8 (n + 1) and the whole input."""
    v = random_values(width, n, seed=77 + in_at + out_at + n)
    same(scan(ctx, v, in_at=in_at, out_at=out_at), reference(v), (width, in_at, out_at, n))


# ---- levels ------------------------------------------------------------------------------------------------------------------------------
def both_limits(ctx, v, small_limit):
    exp = reference(v)
    plain = scan(ctx, v)
    same(plain, exp, "default limit")
    with limit(ctx, small_limit):
        low = scan(ctx, v)
    same(low, exp, f"limit {small_limit}")
    same(low, plain, f"limit {small_limit} against the default")


@pytest.mark.parametrize("small_limit,n", [(2, 3 * TILE + 5), (1, TILE + 1), (4, 4 * TILE), (4, 4 * TILE + 1)])
@pytest.mark.parametrize("width", [4, 8])
def test_levels(ctx, width, small_limit, n):
    """limit 2, 4 block sums: two levels; limit 1, 2 sums: the recursion over 2 values; limit 4 with 4 and with 5 sums: either side of
    the comparison."""
    both_limits(ctx, random_values(width, n, seed=small_limit * 100000 + n + width), small_limit)


def test_three_levels(ctx):
    """4096 * 4096 + 1 items at limit 1: 4097 block sums, then 2, then 1.  64 MB in and 128 MB out, the one large case; at the default
    limit the same input is the one whose 4097 block sums make scan_small_kernel walk 17 rounds of 256 with its carry."""
    both_limits(ctx, random_values(4, TILE * TILE + 1, seed=5), 1)


def test_small_kernel_carries_between_its_rounds(ctx):
    """257 block sums at the default limit: scan_small_kernel's second round of 256 starts from the first one's carry (1 M items)."""
    v = random_values(4, 256 * TILE + 1, seed=6)
    same(scan(ctx, v), reference(v))


def test_option_is_clamped(ctx):
    """Anything above 65536 is 65536, anything <= 0 the default: results never depend on it."""
    v = random_values(4, 2 * TILE + 1, seed=8)
    exp = reference(v)
    try:
        for value in (1 << 40, 65537, 0, -5):
            ctx.set_option("prefix_small_limit", value)
            same(scan(ctx, v), exp, value)
    finally:
        ctx.set_option("prefix_small_limit", 0)


# ---- back to back: the block sums return to the pool while the apply kernel may still read them -------------------------------------------
@pytest.mark.parametrize("sizes", [(TILE * 40 + 3, 5, TILE + 1), (TILE * 256 + 1, TILE * 255 + 9, TILE * 256 + 1)], ids=["sizes_differ", "one_size_class"])
@pytest.mark.parametrize("small_limit", [0, 1])
def test_back_to_back(ctx, small_limit, sizes):
    """Every input and every pattern-filled output is uploaded first (the host waits for those copies).  Then the three scans are
    queued one directly behind the other -- no upload, create, download or wait between the calls -- and only then is anything read
    back: a scan is issued while the one before it may still be running, and takes from the pool the block-sum buffer that scan's
    apply kernel may still be reading.  Stream order is what makes that right.  The pool hands a freed block to a request of up to a
    quarter less than its size class: of 42, 2 and 3 sums the third scan takes the second's block; of 258, 257 and 258 (one class,
    2304 bytes) each takes the block of the one before it, whose apply kernel walks a million items."""
    inputs = [random_values(4, n, seed=900 + i + n) for i, n in enumerate(sizes)]
    jobs = []
    try:
        for v in inputs:
            jobs.append(Job(ctx, v))
        with limit(ctx, small_limit):
            for job in jobs:
                job.launch()
        for job, v in zip(jobs, inputs):
            same(job.sums(), reference(v), (small_limit, len(v)))
    finally:
        for job in jobs:
            job.free()


# ---- wave priority ------------------------------------------------------------------------------------------------------------------------
def test_wave_priority_changes_no_byte():
    from metamdbg_amd import capi
    c = capi.Context(0)
    try:
        v = random_values(4, 5 * TILE + 1021, seed=11)
        got = {}
        for level in (0, 3):
            c.set_option("table_wave_priority", level)
            got[level] = scan(c, v)
            assert c.table_wave_priority() == level
        same(got[0], reference(v), 0)
        assert got[0].tobytes() == got[3].tobytes()
    finally:
        c.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from metamdbg_amd import capi
    L = capi.lib()
    v = random_values(4, 100, seed=12)
    d_in = ctx.bytes_from_host(v.tobytes())                     # 400 bytes
    d_out = ctx.bytes_from_host(bytes(8 * 101))                 # 808 bytes
    both = ctx.bytes_from_host(bytes(4096))

    def refused(rc, word):
        assert rc == -1, rc                                     # MDBG_EINVAL
        msg = (L.mdbg_last_error(ctx.h) or b"").decode()
        assert "mdbg_bytes_prefix_sum" in msg and word in msg, msg

    try:
        assert L.mdbg_bytes_prefix_sum(None, d_in.h, 0, 4, 100, d_out.h, 0) == -1
        refused(L.mdbg_bytes_prefix_sum(ctx.h, None, 0, 4, 100, d_out.h, 0), "null")
        refused(L.mdbg_bytes_prefix_sum(ctx.h, d_in.h, 0, 4, 100, None, 0), "null")
        for width in (0, 1, 2, 3, 5, 16, -4):
            refused(L.mdbg_bytes_prefix_sum(ctx.h, d_in.h, 0, width, 10, d_out.h, 0), "width")
        refused(L.mdbg_bytes_prefix_sum(ctx.h, d_in.h, 2, 4, 10, d_out.h, 0), "in_at")
        refused(L.mdbg_bytes_prefix_sum(ctx.h, d_in.h, 4, 8, 10, d_out.h, 0), "in_at")
        refused(L.mdbg_bytes_prefix_sum(ctx.h, d_in.h, 0, 4, 10, d_out.h, 4), "out_at")
        # a range that leaves its object: one value too many, a start behind the end, a count that wraps 64 bits when multiplied
        refused(L.mdbg_bytes_prefix_sum(ctx.h, d_in.h, 0, 4, 101, both.h, 0), "input")
        refused(L.mdbg_bytes_prefix_sum(ctx.h, d_in.h, 4, 4, 100, both.h, 0), "input")
        refused(L.mdbg_bytes_prefix_sum(ctx.h, d_in.h, 404, 4, 0, both.h, 0), "input")
        refused(L.mdbg_bytes_prefix_sum(ctx.h, d_in.h, 0, 8, 2**61 + 1, both.h, 0), "input")
        refused(L.mdbg_bytes_prefix_sum(ctx.h, both.h, 0, 4, 101, d_out.h, 0), "output")
        refused(L.mdbg_bytes_prefix_sum(ctx.h, d_in.h, 0, 4, 100, d_out.h, 8), "output")
        refused(L.mdbg_bytes_prefix_sum(ctx.h, d_in.h, 0, 4, 0, d_out.h, 808), "output")
        # one object, overlapping ranges: values at [0, 400), sums at [392, 1200); and the sums in front, reaching into the values
        refused(L.mdbg_bytes_prefix_sum(ctx.h, both.h, 0, 4, 100, both.h, 392), "overlap")
        refused(L.mdbg_bytes_prefix_sum(ctx.h, both.h, 800, 4, 100, both.h, 0), "overlap")
        refused(L.mdbg_bytes_prefix_sum(ctx.h, both.h, 0, 8, 10, both.h, 0), "overlap")
        with pytest.raises(capi.MdbgError) as ei:
            ctx.bytes_prefix_sum(d_in, 0, 3, 100, d_out, 0)
        assert ei.value.code == -1
        # the context goes on working: a good call, then one object with ranges that touch but do not overlap
        ctx.bytes_prefix_sum(d_in, 0, 4, 100, d_out, 0)
        same(np.frombuffer(d_out.download(0, 808), dtype="<u8"), reference(v))
        small = np.arange(1, 101, dtype="<u4")
        one = ctx.bytes_from_host(small.tobytes() + bytes(808))
        ctx.bytes_prefix_sum(one, 0, 4, 100, one, 400)
        same(np.frombuffer(one.download(400, 808), dtype="<u8"), reference(small))
        one.free()
    finally:
        for b in (d_in, d_out, both):
            b.free()


def test_no_items_writes_the_total_alone(ctx):
    """n == 0 with out_at 8: one zero, the 8 bytes in front of it and the bytes behind it as they were."""
    for width in (4, 8):
        same(scan(ctx, np.zeros(0, dtype=DTYPE[width]), in_at=0, out_at=8), np.zeros(1, dtype=np.uint64), width)


# ---- one window through the public API: flags, scan, new_off[r] = pos[off[r]] --------------------------------------------------------------
@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193])
def test_apply_density_threshold_offsets_on_the_seams(ctx, orc, n):
    """mdbg_apply_density_threshold is the thinnest caller.  The reads are cut so that an offset falls on 1023, 1024, 4095, 4096, 4097
    (those that exist) and on the total, each twice: an empty read sits at every one of those places."""
    mins = np.arange(n, dtype=np.uint32)
    marks = [m for m in (1023, 1024, 4095, 4096, 4097) if m <= n] + [n]
    offs = np.array(sorted([0] + [m for m in marks for _ in range(2)]), dtype=np.uint64)
    assert offs[0] == 0 and offs[-1] == n and offs[-2] == n
    keep = orc.apply_density_threshold(mins, 0.5)
    assert 0 < len(keep) < n                                    # (the oracle alone: neither nothing nor everything is kept)
    low = ctx.apply_density_threshold(ctx.minimizers_from_host(mins, offs), 0.5).to_host(full=False)
    assert low["offsets"].tolist() == np.searchsorted(keep, offs).tolist()
    assert low["minimizers"].tolist() == mins[keep].tolist()
