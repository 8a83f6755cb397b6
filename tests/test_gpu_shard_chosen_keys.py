"""The owner's side of the sharded passes on rows and keys that are CHOSEN, against tests/shard_model.py.

mdbg_shard_reduce has two forms.  The one-table form (rows_add_kernel / rows_reply_kernel, csrc/shard.hip) is what every small sharded
test runs.  The bucket form (part_owner_reduce, csrc/partition.hip: a radix split of the rows by the top bits of hash_lo, then
owner_bucket_kernel, one workgroup per bucket summing in an LDS table) is taken from 2^17 received rows up, whatever the options say, so
everything here that is to reach it has 2^17 rows or more -- 3 MB.  The rows are uploaded as they stand: any 128-bit key can be fed.

Which form answered is read from the launch timers: every LaunchTimer object named "shard_reduce" is one entry.  The bucket form is one
timed region; the one-table form one per table build plus the reply; a bucket attempt that handed over is the sum of both.  So
"== 1" where the bucket form must answer, "> 1" where it must not, and nothing finer.

The plan of the bucket form (owner_plan, csrc/partition_plan.hpp, whose host test pins the rows below): bits = the least b with
2^b >= n_recv / (0.78 * slots), one split level up to 8 bits, two up to 16.  For the sizes used here:
    n_recv = 2^17      slots 1024: 131072 / 798.72 = 164.1 -> 8 bits, one level     slots 2048: 82.1 -> 7 bits, one level
                       slots  256: 131072 / 199.68 = 656.4 -> 10 bits, two levels (5 + 5)
    n_recv = 300 000   slots 1024: 375.6 -> 9 bits, two levels (5 + 4)   slots 2048: 187.8 -> 8 bits, one   slots 256: 1502.4 -> 11 bits, two
A row's bucket is the top `bits` bits of its hash_lo, its home slot in the bucket's table hash_lo & (slots - 1).
GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from metamdbg_amd import formats
from tests import shard_model as M
from tests.test_gpu_partition import _options
from tests.test_gpu_table_collisions import _zero_word_keys

pytestmark = pytest.mark.gpu

MDBG_EINVAL, MDBG_ERANGE = -1, -5
THRESHOLD = 1 << 17                     # part_owner_reduce: fewer rows than this are the one-table form's
PART_MAX_BITS = 22
SHARD_RPB = 2048                        # rows per block of table_owner_hist_kernel / table_owner_scatter_kernel
FORMS = {"one_table": dict(first_pass_mode=1), "buckets": dict(first_pass_mode=0), "buckets_256": dict(first_pass_mode=0, partition_lds_slots=256),
         "buckets_2048": dict(first_pass_mode=0, partition_lds_slots=2048)}
U64 = np.uint64


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


class _Hip:
    """hipMalloc / hipMemcpy / hipFree of the runtime libmdbg_hip.so has loaded (same SONAME), as test_sharded_first_pass_on_one_gpu uses them."""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so.7")

    def to_device(self, a: np.ndarray) -> C.c_void_p:
        buf = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(buf), C.c_size_t(max(a.nbytes, 8))) == 0
        if a.nbytes:
            assert self.lib.hipMemcpy(buf, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        return buf

    def to_host(self, ptr: int, shape) -> np.ndarray:
        out = np.zeros(shape, dtype=np.uint64)
        if out.nbytes:
            assert self.lib.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self, buf: C.c_void_p) -> None:
        self.lib.hipFree(buf)


@pytest.fixture(scope="module")
def hip(ctx):
    return _Hip()


# ---- the plan of the bucket form, restated ------------------------------------------------------------------------------------

def _plan_bits(n_recv: int, slots: int) -> int:
    bits = 0
    while (1 << bits) < n_recv / (0.78 * (slots or 1024)) and bits <= PART_MAX_BITS:
        bits += 1
    return bits


def _most_keys_in_a_bucket(case, bits: int) -> int:
    """The largest number of distinct keys whose hash_lo share their top `bits` bits."""
    first = np.flatnonzero(case.exp >> U64(63))                           # one row per key
    bucket = (case.rows[first, 0] >> U64(64 - bits)).astype(np.int64) if bits else np.zeros(len(first), dtype=np.int64)
    return int(np.unique(bucket, return_counts=True)[1].max())


# ---- rows ------------------------------------------------------------------------------------------------------------------

class Case:
    """Rows and what the model answers for them: made once, shared by every form, never written to."""

    def __init__(self, rows: np.ndarray):
        self.rows = np.ascontiguousarray(rows, dtype=np.uint64)
        self.exp = M.owner_reply(self.rows)
        _, self.group, self.n_keys = M.key_groups(self.rows)
        for a in (self.rows, self.exp, self.group):
            a.setflags(write=False)


def _rows_of(keys: np.ndarray, counts: np.ndarray, rng) -> np.ndarray:
    rows = np.zeros((len(keys), 3), dtype=np.uint64)
    rows[:, :2] = keys
    rows[:, 2] = counts
    return rows[rng.permutation(len(rows))]


def _random_rows(rng, n: int) -> np.ndarray:
    """n rows: random keys, each arriving 1 to 8 times (as from 8 ranks), random counts, shuffled."""
    n_keys = n // 4 + 64
    keys = rng.integers(1, 1 << 64, (n_keys, 2), dtype=np.uint64)
    idx = np.repeat(np.arange(n_keys), rng.integers(1, 9, n_keys))
    assert len(idx) >= n
    idx = idx[rng.permutation(len(idx))[:n]]
    return _rows_of(keys[idx], rng.integers(1, 1 << 20, n), rng)


def _arrivals(keys: np.ndarray, rng, lo: int, hi: int) -> np.ndarray:
    """Every key lo .. hi - 1 times."""
    return np.repeat(keys, rng.integers(lo, hi, len(keys)), axis=0)


@functools.lru_cache(maxsize=None)
def _case(name: str, slots: int = 0) -> Case:
    rng = np.random.default_rng(sum(name.encode()) * 7 + slots)
    if name.startswith("n="):                                             # (a) sizes around the threshold
        return Case(_random_rows(rng, int(name[2:])))
    if name == "twins":
        # (b) 4096 low words, one in each 4096th of the key space (so any plan of up to 12 bits gives every bucket its share), 16 high
        # words each -- base ^ d with 16 distinct d < 2^17, which also share their home slot in the one-table form (lo ^ (hi >> 17))
        # -- every key three times: 196 608 rows.  Sixteen keys race for one home slot of a bucket's table.
        lo = (np.arange(4096, dtype=np.uint64) << U64(52)) | rng.integers(1, 1 << 52, 4096, dtype=np.uint64)
        base = rng.integers(1 << 20, 1 << 64, 4096, dtype=np.uint64)
        d = (rng.integers(0, 1 << 13, (4096, 16)) + (np.arange(16) << 13)).astype(np.uint64)
        keys = np.stack([np.repeat(lo, 16), (base[:, None] ^ d).reshape(-1)], 1)
        keys = np.repeat(keys, 3, axis=0)
        return Case(_rows_of(keys, rng.integers(1, 1 << 20, len(keys)), rng))
    if name == "wrap":
        # (c) in six buckets of ANY plan up to 11 bits (hash_lo sharing its top 11 bits; the first and the last bucket among them)
        # slots / 2 distinct keys whose hash_lo ends in 0x7FC .. 0x7FF: the last four slots of a table of 256, 1024 or 2048 slots alike,
        # so every probe chain of theirs runs round the table's end.  Around them 2^17 random rows.
        per = (slots or 1024) // 2
        parts = [_random_rows(rng, THRESHOLD)]
        for top in (0, 300, 700, 1100, 1500, 2047):                           # (apart in their top 7 bits: six buckets of any plan here)
            lo = (U64(top) << U64(53)) | (rng.integers(0, 1 << 42, per, dtype=np.uint64) << U64(11)) | (U64(0x7FC) + rng.integers(0, 4, per).astype(np.uint64))
            keys = np.unique(np.stack([lo, rng.integers(1, 1 << 64, per, dtype=np.uint64)], 1), axis=0)
            keys = _arrivals(keys, rng, 1, 5)
            parts.append(_rows_of(keys, rng.integers(1, 1 << 20, len(keys)), rng))
        rows = np.concatenate(parts)
        return Case(rows[rng.permutation(len(rows))])
    if name == "one_key":
        # (d) 2^17 rows of one key: one bucket takes every row, every other is empty; counts below 2^15, the total below 2^32
        rows = np.zeros((THRESHOLD, 3), dtype=np.uint64)
        rows[:, 0], rows[:, 1] = 0x0123456789ABCDEF, 0xFEDCBA9876543210
        rows[:, 2] = rng.integers(1, 1 << 15, THRESHOLD)
        return Case(rows)
    if name == "bit31":
        # (e) every key three rows that sum to a value in [2^31, 2^32)
        menu = np.array([(0x7FFFFFFF, 0x7FFFFFFF, 1), (0x80000000, 0, 0), (0xFFFFFFFF, 0, 0), (0x40000000, 0x40000000, 0x40000000),
                         (0x7FFFFFFF, 1, 0x7FFFFFFF), (1, 0xFFFFFFFD, 1), (0x55555555, 0x55555555, 0x55555555)], dtype=np.uint64)
        n_keys = THRESHOLD // 3 + 1
        keys = rng.integers(1, 1 << 64, (n_keys, 2), dtype=np.uint64)
        counts = menu[rng.integers(0, len(menu), n_keys)]
        return Case(_rows_of(np.repeat(keys, 3, axis=0), counts.reshape(-1), rng))
    if name == "no_fit":
        # (f) 2100 distinct keys whose hash_lo share their top 22 bits (PART_MAX_BITS: no plan separates them; the largest table has
        # 2048 slots), each once to three times, among 2^17 random rows
        lo = (U64(0x2ABCDE) << U64(42)) | rng.integers(0, 1 << 42, 2100, dtype=np.uint64)
        keys = _arrivals(np.stack([lo, rng.integers(1, 1 << 64, 2100, dtype=np.uint64)], 1), rng, 1, 4)
        rows = np.concatenate([_random_rows(rng, THRESHOLD), _rows_of(keys, rng.integers(1, 1 << 20, len(keys)), rng)])
        return Case(rows[rng.permutation(len(rows))])
    if name in ("zero_words_64", "zero_words_65"):
        # (g) (0, h), (l, 0) and (0, 0) -- the variants of test_zero_word_keys -- 64 distinct keys (TABLE_EXC_CAP: what the side list
        # holds; a condition of the test) or 65, each two to five times, among 2^17 random rows
        keys = _arrivals(_zero_word_keys(rng, int(name[-2:])), rng, 2, 6)
        rows = np.concatenate([_random_rows(rng, THRESHOLD), _rows_of(keys, rng.integers(1, 1 << 20, len(keys)), rng)])
        return Case(rows[rng.permutation(len(rows))])
    if name == "distinct":
        # (h) 2^17 rows, every key once
        return Case(_rows_of(rng.integers(1, 1 << 64, (THRESHOLD, 2), dtype=np.uint64), rng.integers(1, 1 << 20, THRESHOLD), rng))
    if name == "small":
        # an ordinary call: 5000 rows, three zero-word keys among them
        keys = _arrivals(np.array([(0, 77), (77, 0), (0, 0)], dtype=np.uint64), rng, 2, 4)
        rows = np.concatenate([_random_rows(rng, 5000), _rows_of(keys, rng.integers(1, 1 << 20, len(keys)), rng)])
        return Case(rows[rng.permutation(len(rows))])
    raise KeyError(name)


# ---- the call and the check ---------------------------------------------------------------------------------------------------

def _reduce(ctx, hip, rows: np.ndarray, form: str, n_ranks: int = 1):
    """mdbg_shard_reduce over `rows` on a fresh shard (begun over an empty minimizer set) in the given form:
    (replies u64[n], launch entries named "shard_reduce")."""
    empty = ctx.minimizers_from_host(np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64))
    sh, buf = None, None
    try:
        _options(ctx, **FORMS[form])
        sh = ctx.shard_begin(empty, 4, n_ranks)
        assert sh.n_rows == 0
        buf = hip.to_device(rows)
        ctx.timing(True)
        ctx.timing_reset()
        d_reply = sh.reduce(buf.value, len(rows))
        launches = ctx.timing_get("shard_reduce")[1]
        return hip.to_host(d_reply, (len(rows),)), launches
    finally:
        ctx.timing(False)
        ctx.timing_reset()
        _options(ctx)
        if sh is not None:
            sh.free()
        if buf is not None:
            hip.free(buf)
        empty.free()


def _show(case: Case, bad: np.ndarray, reply: np.ndarray):
    return [(int(i), hex(int(case.rows[i, 0])), hex(int(case.rows[i, 1])), int(case.rows[i, 2]), hex(int(reply[i])), hex(int(case.exp[i]))) for i in bad[:6]]


def _check_reply(case: Case, reply: np.ndarray, lister_is_first_row: bool):
    count, flag = reply & M.COUNT_MASK, reply >> U64(63)
    bad = np.flatnonzero(count != (case.exp & M.COUNT_MASK))
    assert len(bad) == 0, ("counts (row, lo, hi, count, reply, model)", len(bad), _show(case, bad, reply))
    bad = np.flatnonzero((reply >> U64(32)) & U64(0x7FFFFFFF))
    assert len(bad) == 0, ("bits 32..62", len(bad), _show(case, bad, reply))
    listers = np.bincount(case.group[flag == 1], minlength=case.n_keys)
    bad_keys = np.flatnonzero(listers != 1)
    assert len(bad_keys) == 0, ("listers per key", len(bad_keys), [(int(g), int(listers[g]), _show(case, np.flatnonzero(case.group == g), reply)) for g in bad_keys[:3]])
    if lister_is_first_row:                                               # owner_bucket_kernel: atomicMin over the key's row indices
        bad = np.flatnonzero(flag != (case.exp >> U64(63)))
        assert len(bad) == 0, ("the lister is not the key's first row", len(bad), _show(case, bad, reply))


def _run(ctx, hip, case: Case, form: str, buckets_answer: bool, n_ranks: int = 1):
    reply, launches = _reduce(ctx, hip, case.rows, form, n_ranks)
    print(f"{len(case.rows)} rows, {case.n_keys} keys, form {form}: {launches} launch entries of shard_reduce")
    if buckets_answer:
        assert launches == 1, launches
    else:
        assert launches > 1, launches
    _check_reply(case, reply, buckets_answer)


def _slots(form: str) -> int:
    return FORMS[form].get("partition_lds_slots", 0)


def _fits(case: Case, form: str) -> bool:
    """Every bucket of the form's plan holds its keys at a load of at most 0.78 (the keys have no zero word)."""
    slots = _slots(form) or 1024
    return _most_keys_in_a_bucket(case, _plan_bits(len(case.rows), slots)) <= 0.78 * slots


# ---- 2. mdbg_shard_reduce against the model -------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [THRESHOLD - 1, THRESHOLD, THRESHOLD + 1, 300_000])
def test_sizes_around_the_threshold(ctx, hip, n, form):
    """(a) 2^17 - 1 rows are the one-table form's even in mode 0; from 2^17 on the bucket form answers: one split level with 1024 and 2048
    slots and two with 256 at 2^17 (+ 1), two levels with 1024 slots as well at 300 000 (the module's docstring derives them)."""
    case = _case(f"n={n}")
    assert len(case.rows) == n
    _run(ctx, hip, case, form, buckets_answer=form != "one_table" and n >= THRESHOLD)


@pytest.mark.parametrize("form", FORMS)
def test_low_word_twins(ctx, hip, form):
    """(b) sixteen keys of one low word, 4096 times over, every key three times, shuffled: the claim of an LDS slot by its low word
    says nothing about whose slot it becomes (lds_slot: CAS on the low word, the high word published separately)."""
    case = _case("twins")
    assert len(case.rows) == 196608 and case.n_keys == 65536 and _fits(case, form)
    _run(ctx, hip, case, form, buckets_answer=form != "one_table")


@pytest.mark.parametrize("form", FORMS)
def test_clusters_that_wrap_at_the_tables_end(ctx, hip, form):
    """(c) half a table of keys whose home is one of its last four slots, in six buckets: lds_slot and lds_find walk round the end."""
    slots = _slots(form) or 1024
    case = _case("wrap", slots)
    lo = case.rows[:, 0]
    in_cluster = (lo & U64(0x7FC)) == U64(0x7FC)
    assert int(in_cluster.sum()) >= 6 * (slots // 2) and _fits(case, form)
    assert _plan_bits(len(case.rows), slots) <= 11                         # the clusters' keys do share a bucket
    _run(ctx, hip, case, form, buckets_answer=form != "one_table")


@pytest.mark.parametrize("form", FORMS)
def test_one_key_only(ctx, hip, form):
    """(d) 2^17 rows of the same key: one slot, one bucket (a segment that one block of the second level splits alone), row 0 lists."""
    case = _case("one_key")
    assert case.n_keys == 1 and int(case.exp[0]) >> 63 == 1 and int(case.rows[:, 2].sum()) < 1 << 32
    _run(ctx, hip, case, form, buckets_answer=form != "one_table")


@pytest.mark.parametrize("form", FORMS)
def test_totals_with_bit_31_set(ctx, hip, form):
    """(e) every total in [2^31, 2^32): nothing may be taken for a sign, and nothing may reach bits 32 .. 62."""
    case = _case("bit31")
    assert int((case.exp & M.COUNT_MASK).min()) >= 1 << 31 and _fits(case, form)
    _run(ctx, hip, case, form, buckets_answer=form != "one_table")


@pytest.mark.parametrize("form", FORMS)
def test_a_bucket_that_cannot_fit_hands_over(ctx, hip, form):
    """(f) more keys in one bucket of the deepest plan there is than the largest table has slots: PART_OVERFLOW_TABLE, the one-table
    form takes the rows over and the answer is the model's all the same.  (To the one-table form these keys were 2100 in six home
    slots -- its home is the top bits of lo ^ (hi >> 17), the first 17 of them hash_lo's -- and the call ended in "hash table
    overflow" in every form, as (c) did in mode 1, until rows_add_kernel / rows_reply_kernel keyed the owner's table by fmix64(hash_lo).)"""
    case = _case("no_fit")
    assert _most_keys_in_a_bucket(case, PART_MAX_BITS) > 2048
    _run(ctx, hip, case, form, buckets_answer=False)


@pytest.mark.parametrize("form", FORMS)
def test_zero_word_keys_hand_over(ctx, hip, form):
    """(g) 64 distinct keys with a zero word among 2^17 random rows: PART_OVERFLOW_ZERO_KEY, and the side list of the one-table form
    holds exactly that many."""
    case = _case("zero_words_64")
    zero = (case.rows[:, 0] == 0) | (case.rows[:, 1] == 0)
    assert len(np.unique(case.rows[zero, :2], axis=0)) == 64 and int(zero.sum()) >= 128
    _run(ctx, hip, case, form, buckets_answer=False)


@pytest.mark.parametrize("form", FORMS)
def test_more_zero_word_keys_than_the_side_list_holds(ctx, hip, form):
    """65 of them: the library's clean error (what test_the_two_limits_are_clean_errors asserts for mdbg_prev_from_records), and a
    correct call straight afterwards succeeds."""
    from metamdbg_amd import capi
    case = _case("zero_words_65")
    with pytest.raises(capi.MdbgError) as e:
        _reduce(ctx, hip, case.rows, form)
    assert e.value.code == MDBG_ERANGE and "overflow" in str(e.value)
    _run(ctx, hip, _case("small"), form, buckets_answer=False)


def test_the_one_table_form_grows_and_refills(ctx, hip):
    """(h) 2^17 distinct keys on a shard begun for 64 ranks: mdbg_shard_reduce expects n / 64 * 1.5 + 1024 = 4096 keys and sizes the
    table for them (some 2 * 10^4 slots), so the table must grow and the rows go in again."""
    case = _case("distinct")
    assert case.n_keys == THRESHOLD
    _run(ctx, hip, case, "one_table", buckets_answer=False, n_ranks=64)


# ---- 3. grouping by owner: mdbg_shard_from_table ----------------------------------------------------------------------------------

def _records(keys: np.ndarray, ab: np.ndarray) -> np.ndarray:
    rec = np.zeros(len(keys), dtype=formats.ABUNDANCE_DTYPE)
    rec["lo"], rec["hi"], rec["abundance"] = keys[:, 0], keys[:, 1], ab
    return rec


def _boundary_keys(n_ranks: int, rng) -> np.ndarray:
    """For every owner j the two values of hi >> 32 either side of its lower boundary -- ceil(j 2^32 / n) - 1 and ceil(j 2^32 / n) --
    and 0 and 2^32 - 1; each with a low half of hi of all zeros, all ones and random (it must not matter); hash_lo random."""
    tops = {0, 0xFFFFFFFF}
    for c in M.owner_first_tops(n_ranks):
        tops.update({c, max(c - 1, 0)})
    hi = []
    for t in sorted(tops):
        hi += [(t << 32) | low for low in (0, 0xFFFFFFFF, int(rng.integers(1, 0xFFFFFFFF)))]
    hi = np.array(hi, dtype=np.uint64)
    return np.stack([rng.integers(1, 1 << 64, len(hi), dtype=np.uint64), hi], 1)


def _sorted_rows(rows: np.ndarray) -> np.ndarray:
    return rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]


@pytest.mark.parametrize("n_ranks", [1, 2, 3, 5, 7, 8, 63, 64])
def test_grouping_by_owner(ctx, hip, n_ranks):
    """Tables of 1, 2047, 2048, 2049 and 3 * 2048 + 5 rows (SHARD_RPB = 2048 rows a block) from records whose keys sit on the owner
    boundaries: the table keeps the records as uploaded; the counts per owner are the model's; every row lies in its owner's
    segment; the rows are the table's, each once."""
    rng = np.random.default_rng(300 + n_ranks)
    edge = _boundary_keys(n_ranks, rng)
    assert len(np.unique(edge, axis=0)) == len(edge) < SHARD_RPB - 1      # every boundary key is in every table but the first
    for n_rows in (1, SHARD_RPB - 1, SHARD_RPB, SHARD_RPB + 1, 3 * SHARD_RPB + 5):
        keys = np.concatenate([edge, rng.integers(1, 1 << 64, (max(0, n_rows - len(edge)), 2), dtype=np.uint64)])
        keys = keys[rng.permutation(len(keys))[:n_rows]]
        rec = _records(keys, rng.integers(1, 1 << 32, n_rows, dtype=np.uint64).astype(np.uint32))
        table = ctx.prev_from_records(rec)
        got, _ = table.to_host()
        assert got.tobytes() == rec.tobytes()
        sh = ctx.shard_from_table(table, n_ranks)
        try:
            rows = hip.to_host(sh.d_rows, (n_rows, 3))
            own = M.owner_of(rec["hi"], n_ranks)
            want = np.bincount(own, minlength=n_ranks)
            assert sh.n_rows == n_rows and np.array_equal(np.asarray(sh.counts, dtype=np.int64), want), (n_rows, sh.counts, want)
            segment = np.repeat(np.arange(n_ranks), want)
            bad = np.flatnonzero(M.owner_of(rows[:, 1], n_ranks) != segment)
            assert len(bad) == 0, (n_rows, [(int(i), hex(int(rows[i, 1])), int(segment[i])) for i in bad[:6]])
            mine = np.stack([rec["lo"], rec["hi"], rec["abundance"].astype(np.uint64)], 1)
            assert np.array_equal(_sorted_rows(rows), _sorted_rows(mine)), n_rows
        finally:
            sh.free()
            table.free()


def test_rank_counts_out_of_range_are_refused(ctx, hip):
    """n_ranks 0 and 65 (the kernels keep one counter per owner in h[64]): MDBG_EINVAL, and a correct call afterwards works."""
    from metamdbg_amd import capi
    rng = np.random.default_rng(7)
    rec = _records(rng.integers(1, 1 << 64, (500, 2), dtype=np.uint64), rng.integers(1, 900, 500).astype(np.uint32))
    table = ctx.prev_from_records(rec)
    for n_ranks in (0, 65):
        with pytest.raises(capi.MdbgError) as e:
            ctx.shard_from_table(table, n_ranks)
        assert e.value.code == MDBG_EINVAL
        sh = ctx.shard_from_table(table, 64)
        rows = hip.to_host(sh.d_rows, (500, 3))
        assert np.array_equal(np.asarray(sh.counts, dtype=np.int64), np.bincount(M.owner_of(rec["hi"], 64), minlength=64))
        assert np.array_equal(_sorted_rows(rows), _sorted_rows(np.stack([rec["lo"], rec["hi"], rec["abundance"].astype(np.uint64)], 1)))
        sh.free()
    table.free()


# ---- 4. the chain: shard_from_table -> exchange_local -> keep ----------------------------------------------------------------------

POOL = 180_000                          # keys; a rank holds 0.8 of them, so every owner receives some 144 000 rows, whatever the rank count


class Chain:
    pass


@functools.lru_cache(maxsize=None)
def _chain(n_ranks: int) -> Chain:
    """One pool of keys -- random ones, 2500 groups of eight twins (one lo; hi = base ^ d, d < 2^17: one owner unless they straddle a
    boundary), the owner boundaries of this rank count, seven zero-word keys, all of them owner 0's -- and per rank a random 0.8 of it
    in a random order with abundances of the rank's own."""
    rng = np.random.default_rng(900 + n_ranks)
    lo = rng.integers(1, 1 << 64, 2500, dtype=np.uint64)
    base = rng.integers(1 << 20, 1 << 64, 2500, dtype=np.uint64)
    d = (rng.integers(0, 1 << 14, (2500, 8)) + (np.arange(8) << 14)).astype(np.uint64)
    twins = np.stack([np.repeat(lo, 8), (base[:, None] ^ d).reshape(-1)], 1)
    zero = np.array([(0, 0), (0, 1), (0, 0xFFFFFFFF), (0, 12345), (1, 0), (1 << 63, 0), (0xFFFFFFFFFFFFFFFF, 0)], dtype=np.uint64)
    assert (M.owner_of(zero[:, 1], n_ranks) == 0).all()
    edge = _boundary_keys(n_ranks, rng)
    edge = edge[edge[:, 1] != 0]
    keys = np.concatenate([twins, zero, edge])
    keys = np.concatenate([keys, rng.integers(1, 1 << 64, (POOL - len(keys), 2), dtype=np.uint64)])
    assert len(np.unique(keys, axis=0)) == POOL
    S = Chain()
    S.keys = keys
    S.order = np.lexsort((keys[:, 0], keys[:, 1]))
    S.sorted_lo, S.sorted_hi = keys[S.order, 0], keys[S.order, 1]
    S.longest_run = int(np.unique(S.sorted_hi, return_counts=True)[1].max())
    S.held = rng.random((n_ranks, POOL)) < 0.8
    S.ab = rng.integers(1, 1 << 32, (n_ranks, POOL), dtype=np.uint64).astype(np.uint32)
    S.ids = [rng.permutation(np.flatnonzero(S.held[r])) for r in range(n_ranks)]
    S.records = [_records(keys[i], S.ab[r, i]) for r, i in enumerate(S.ids)]
    own = M.owner_of(keys[:, 1], n_ranks)
    S.received = np.array([int(S.held[:, own == j].sum()) for j in range(n_ranks)])
    return S


def _pool_ids(S: Chain, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """The pool index of every (lo, hi), -1 for a key that is not in the pool."""
    lo, hi = lo.astype(np.uint64), hi.astype(np.uint64)
    first = np.searchsorted(S.sorted_hi, hi, "left")
    ids = np.full(len(lo), -1, dtype=np.int64)
    for t in range(S.longest_run):                                        # the few keys of one hi stand side by side
        at = np.minimum(first + t, POOL - 1)
        hit = (S.sorted_hi[at] == hi) & (S.sorted_lo[at] == lo)
        ids[hit] = S.order[at[hit]]
    return ids


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n_ranks", [2, 3, 8])
def test_chain_on_chosen_keys(ctx, n_ranks, mode):
    """mdbg_shard_from_table -> mdbg_shard_exchange_local -> mdbg_shard_keep over tables that overlap: every key some rank holds is
    kept by exactly one rank, which holds it, with that rank's own abundance (keep_rows_kernel copies the local row), and nothing else is
    kept.  Every owner receives 2^17 rows or more, so in mode 0 the bucket form answers inside the exchange (owner 0, which has the
    zero-word keys, through the hand-over)."""
    from metamdbg_amd import capi
    S = _chain(n_ranks)
    assert (S.received >= THRESHOLD).all(), S.received
    tables, shards, kept = [], [], []
    try:
        _options(ctx, first_pass_mode=mode)
        tables = [ctx.prev_from_records(rec) for rec in S.records]        # (alive until keep has returned: the shards point into them)
        shards = [ctx.shard_from_table(t, n_ranks) for t in tables]
        for r, sh in enumerate(shards):
            assert sh.n_rows == len(S.ids[r])
        assert np.array_equal(np.sum([np.asarray(sh.counts, dtype=np.int64) for sh in shards], axis=0), S.received)
        replies = capi.exchange_local(ctx, shards)
        kept = [sh.keep(p) for sh, p in zip(shards, replies)]
        recs = [t.to_host()[0] for t in kept]
    finally:
        _options(ctx)
        for x in kept + tables:
            x.free()
        for sh in shards:
            sh.free()
    times_kept = np.zeros(POOL, dtype=np.int64)
    for r, rec in enumerate(recs):
        ids = _pool_ids(S, rec["lo"], rec["hi"])
        assert (ids >= 0).all(), (r, "a key that is in no table")
        assert S.held[r, ids].all(), (r, "a key this rank does not hold")
        bad = np.flatnonzero(rec["abundance"] != S.ab[r, ids])
        assert len(bad) == 0, (r, "not the rank's own abundance", [(int(i), int(rec["abundance"][i]), int(S.ab[r, ids[i]])) for i in bad[:6]])
        times_kept += np.bincount(ids, minlength=POOL)
    assert np.array_equal(times_kept, S.held.any(axis=0).astype(np.int64)), np.flatnonzero(times_kept != S.held.any(axis=0))[:10]
