"""What the owner's side of a sharded pass must answer, in vectorised numpy (64-bit integers throughout): the model the GPU tests of
tests/test_gpu_shard_chosen_keys.py hold mdbg_shard_reduce / mdbg_shard_from_table against.  The loop versions in
tests/test_distributed_gloo.py say the same and are what tests/test_shard_model.py checks these against; they take minutes for the
2^17 rows and more at which the bucket form of the reduction (csrc/partition.hip, part_owner_reduce) engages."""
from __future__ import annotations

import numpy as np

EMIT_BIT = np.uint64(1 << 63)
COUNT_MASK = np.uint64(0xFFFFFFFF)


def owner_of(hi, n_ranks: int) -> np.ndarray:
    """csrc/shard.hip owner_of: ((hi >> 32) * n_ranks) >> 32, the top half of hash_hi scaled to [0, n_ranks)."""
    hi = np.asarray(hi).astype(np.uint64, copy=False)
    return (((hi >> np.uint64(32)) * np.uint64(n_ranks)) >> np.uint64(32)).astype(np.int64)


def owner_first_tops(n_ranks: int) -> list[int]:
    """The smallest hi >> 32 that owner j has, for every j: ceil(j * 2^32 / n_ranks)."""
    return [-((-j << 32) // n_ranks) for j in range(n_ranks)]


def _rows_u64(rows) -> np.ndarray:
    r = np.ascontiguousarray(rows)
    assert r.ndim == 2 and r.shape[1] == 3 and r.dtype.itemsize == 8
    return r.view(np.uint64)


def key_groups(rows) -> tuple[np.ndarray, np.ndarray, int]:
    """(order, group, n_keys): `order` sorts the rows by key with equal keys in the order they arrived, group[i] numbers row i's key."""
    u = _rows_u64(rows)
    n = len(u)
    order = np.lexsort((u[:, 0], u[:, 1]))                 # stable: rows of one key keep their order
    group = np.zeros(n, dtype=np.int64)
    if n == 0:
        return order, group, 0
    lo, hi = u[order, 0], u[order, 1]
    new = np.ones(n, dtype=bool)
    new[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    sorted_group = np.cumsum(new) - 1
    group[order] = sorted_group
    return order, group, int(sorted_group[-1]) + 1


def owner_reply(rows) -> np.ndarray:
    """uint64[n]: the low 32 bits are the sum of the key's counts modulo 2^32 (both device forms add in uint32_t, the reference's
    abundance is a u32), bit 63 is set on the key's first row, nothing else is set."""
    u = _rows_u64(rows)
    n = len(u)
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    order, group, n_keys = key_groups(u)
    starts = np.flatnonzero(np.diff(group[order], prepend=-1))
    # (counts are reduced to 32 bits first, as the device reads them: 2^32 rows of less than 2^32 each cannot overflow a u64)
    total = np.add.reduceat(u[order, 2] & COUNT_MASK, starts) & COUNT_MASK
    out = total[group]
    out[order[starts]] |= EMIT_BIT
    return out
