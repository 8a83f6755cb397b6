"""tests/shard_model.py (vectorised, what the GPU tests use) against the loop versions the CPU exchange tests use
(tests/test_distributed_gloo.py: owner_reply, owner_of), on rows with duplicates, low-word twins, zero-word keys and the owner
boundaries of every rank count tests/test_gpu_shard_chosen_keys.py runs."""
from __future__ import annotations

import numpy as np
import pytest

from tests import shard_model as M
from tests.test_distributed_gloo import owner_of as loop_owner_of
from tests.test_distributed_gloo import owner_reply as loop_owner_reply

RANKS = [1, 2, 3, 5, 7, 8, 63, 64]


def _boundary_his(n_ranks, rng):
    """hi whose top half is the last value of owner j - 1 and the first of owner j, for every j, and 0 and 2^32 - 1; the low half is
    0, all ones and random."""
    tops = {0, 0xFFFFFFFF}
    for c in M.owner_first_tops(n_ranks):
        tops.update({c, max(c - 1, 0)})
    out = []
    for t in sorted(tops):
        out += [t << 32, (t << 32) | 0xFFFFFFFF, (t << 32) | int(rng.integers(1, 0xFFFFFFFF))]
    return np.array(out, dtype=np.uint64)


@pytest.mark.parametrize("n_ranks", RANKS)
def test_owner_of_matches_the_loop_version_and_its_definition(n_ranks):
    rng = np.random.default_rng(n_ranks)
    hi = np.concatenate([_boundary_his(n_ranks, rng), rng.integers(0, 1 << 64, 500, dtype=np.uint64)])
    got = M.owner_of(hi, n_ranks)
    assert np.array_equal(got, loop_owner_of(hi, n_ranks))
    assert got.tolist() == [((int(h) >> 32) * n_ranks) >> 32 for h in hi]          # exact integers
    assert got.min() == 0 and got.max() == n_ranks - 1
    # the boundaries are where they are said to be: owner j starts at ceil(j 2^32 / n)
    for j, c in enumerate(M.owner_first_tops(n_ranks)):
        assert int(M.owner_of(np.array([c << 32], dtype=np.uint64), n_ranks)[0]) == j
        if j:
            assert int(M.owner_of(np.array([((c - 1) << 32) | 0xFFFFFFFF], dtype=np.uint64), n_ranks)[0]) == j - 1


def _rows(rng, n_ranks):
    """Some 3000 rows: random keys arriving 1 to 8 times, twins (one lo, several hi) arriving several times each, keys with a zero
    word, the boundary values of hi; counts small, large, and summing past 2^31; shuffled."""
    keys = rng.integers(1, 1 << 64, (300, 2), dtype=np.uint64)
    twin_lo = rng.integers(1, 1 << 64, 20, dtype=np.uint64)
    twins = np.stack([np.repeat(twin_lo, 6), rng.integers(1, 1 << 64, 120, dtype=np.uint64)], 1)
    zero = np.array([(0, 5), (5, 0), (0, 0), (0, 1 << 63), (1 << 63, 0)], dtype=np.uint64)
    bh = _boundary_his(n_ranks, rng)
    bound = np.stack([rng.integers(1, 1 << 64, len(bh), dtype=np.uint64), bh], 1)
    keys = np.concatenate([keys, twins, zero, bound])
    keys = np.repeat(keys, rng.integers(1, 9, len(keys)), axis=0)
    rows = np.zeros((len(keys), 3), dtype=np.uint64)
    rows[:, :2] = keys
    rows[:, 2] = rng.integers(1, 1000, len(keys))
    big = rng.random(len(keys)) < 0.1
    rows[big, 2] = rng.integers(1 << 27, 1 << 28, int(big.sum()))         # at most 8 rows a key: these totals stay below 2^31
    # totals with bit 31 set (the loop version does not reduce modulo 2^32: none goes past it)
    top = np.array([(11, 12, 0x7FFFFFFF), (11, 12, 0x7FFFFFFF), (11, 12, 1), (11, 13, 0x80000000), (11, 14, 0xFFFFFFFF)], dtype=np.uint64)
    rows = np.concatenate([rows, top])
    return rows[rng.permutation(len(rows))]


@pytest.mark.parametrize("n_ranks", RANKS)
def test_owner_reply_matches_the_loop_version(n_ranks):
    rng = np.random.default_rng(100 + n_ranks)
    rows = _rows(rng, n_ranks)
    want = loop_owner_reply(rows.view(np.int64)).view(np.uint64)
    got = M.owner_reply(rows)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert np.array_equal(M.owner_reply(rows.view(np.int64)), want)      # rows as the exchange carries them
    assert (want & M.COUNT_MASK).max() >= 1 << 31                         # totals with bit 31 set are among them
    order, group, n_keys = M.key_groups(rows)
    assert n_keys == len(set(map(tuple, rows[:, :2].tolist())))
    assert np.array_equal(np.bincount(group[(got >> np.uint64(63)) == 1], minlength=n_keys), np.ones(n_keys, dtype=np.int64))


def test_owner_reply_adds_modulo_2_32_and_takes_no_rows():
    rows = np.array([(7, 9, 0xFFFFFFFF), (7, 9, 2), (7, 8, 0x7FFFFFFF), (7, 8, 0x7FFFFFFF), (7, 8, 1), (7, 9, 1 << 32)], dtype=np.uint64)
    assert M.owner_reply(rows).tolist() == [(1 << 63) | 1, 1, (1 << 63) | 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 1]
    assert len(M.owner_reply(np.zeros((0, 3), dtype=np.uint64))) == 0
