"""The read sets of tests/rescue_model.py, checked without a GPU: the plain-Python restatement of the rescue rule and the C oracle give the
same rescued rows in the same order, and every set holds the cases it was built for (conditions on the inputs, not measurements).
Run with -s to see the verdict census of each set."""
from __future__ import annotations

import numpy as np
import pytest

from tests import rescue_model as M

N_CU = 256                                       # the sweep floor below is restated by the GPU test with the device's own figure


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _check(orc, rows, k: int, name: str):
    mins, offs = M.to_arrays(rows)
    model, verdicts, n_rows = M.rescued_rows(rows, k, 0)
    exp = orc.kminmer_count_first(mins, offs, k, 0)
    got = M.canonical_rows(exp["vecs"][exp["n_solid"]:])
    assert got == model, f"{name} k={k}: the model and the oracle differ"
    e = orc.kminmer_count_first(mins, offs, k, 1)                # the model does not look at min_abundance below 2
    assert M.canonical_rows(e["vecs"][e["n_solid"]:]) == model
    e = orc.kminmer_count_first(mins, offs, k, 2)
    assert len(e["vecs"]) == e["n_solid"] and M.rescued_rows(rows[:2000], k, 2)[0] == []
    c = M.census(rows, verdicts, k)
    print(f"\n{name} k={k}: {len(rows)} reads, {len(mins)} minimizers, {len(model)} rescued rows; " +
          ", ".join(f"{v}: {n}" for v, n in c.items() if n))
    assert len(mins) < 1_500_000
    return c, verdicts, n_rows


@pytest.mark.parametrize("k", M.KS)
def test_battery(orc, k):
    rows = M.dataset("battery", k)
    c, verdicts, n_rows = _check(orc, rows, k, "battery")
    assert c["tie-rescued"] >= 20 and c["tie-not"] >= 20 and c["rescued n>16"] >= 20 and c["not n>16"] >= 20 and c["all ones"] >= 16
    # rescued reads without a row: no window seen once
    assert sum(1 for v, n in zip(verdicts, n_rows) if v.endswith("rescued") and n == 0) >= 20
    # counts of 254 and above are there
    from collections import Counter
    assert {254, 255, 256, 300} <= set(Counter(w for r in rows for w in M._windows(r, k)).values())
    keys, inst = M.keys_and_instances(rows, k)
    assert keys <= 0.25 * inst                               # the partitioned form's byte array starts from "many"


@pytest.mark.parametrize("k", (3, 4))
def test_quadruples(orc, k):
    rows = M.dataset("quadruples", k)
    c, verdicts, _ = _check(orc, rows, k, "quadruples")
    # the first 24 reads are the six hand-laid waves, 50 times over
    assert verdicts[0:4] == ["tie-rescued", "tie-not", "rescued", "not"]
    assert all(v.startswith("tie-") for v in verdicts[4:8]) and len(set(verdicts[4:8])) == 2
    assert verdicts[8:12] == ["no windows", "tie-rescued", "no windows", "all ones"]
    assert verdicts[12:16] == ["all ones", "no windows", "tie-not", "no windows"]
    assert verdicts[16:20] == ["tie-rescued", "tie-rescued", "all ones", "tie-not"] and len(rows[17]) - k + 1 == 100
    assert verdicts[20:24] == ["tie-not", "rescued", "tie-not", "tie-not"] and len(rows[23]) - k + 1 == 100
    assert all(verdicts[i: i + 24] == verdicts[:24] for i in range(0, 24 * 50, 24))


def test_quadruples_more_than_two_sweeps(orc):
    floor = 2 * N_CU * 16 * 16
    rows = M.dataset("quadruples_sweeps", 3, floor)
    _check(orc, rows, 3, "quadruples_sweeps")
    assert len(rows) > floor and len(rows) % (N_CU * 16 * 16) != 0       # several trips of the r0 loop, dead groups in the last


@pytest.mark.parametrize("k", (3, 4, 33))
def test_prefixes(orc, k):
    want = ["tie-not", "tie-rescued", "no windows", "rescued", "all ones"]
    for n in (1, 2, 3, 5):
        rows = M.dataset("prefix", k, n)
        _, verdicts, n_rows = _check(orc, rows, k, f"prefix {n}")
        assert verdicts == want[:n] and n_rows == [0, 11, 0, 40, 0][:n]


@pytest.mark.parametrize("k", (3, 4, 13))
def test_row_order(orc, k):
    rows = M.dataset("row_order", k)
    c, verdicts, n_rows = _check(orc, rows, k, "row_order")
    # neighbours differ: among the pattern pairs, a rescued read with rows sits beside one that is left alone
    pairs = [(verdicts[i], verdicts[i + 1]) for i in range(0, 2 * sum(len(M.weak_patterns(n)) for n in (16, 17, 33, 100)), 2)]
    assert sum(1 for a, b in pairs if a.endswith("rescued") and b.endswith("not")) >= 12
    # a weak palindromic window and weak windows stored reversed are among the rows
    model = M.rescued_rows(rows, k, 0)[0]
    assert sum(1 for w in model if w == w[::-1]) >= 9
    reversed_rows = 0
    for r, v, n in zip(rows, verdicts, n_rows):
        reversed_rows += n if n and len(r) > k and r[0] > r[1] else 0
    assert reversed_rows >= 20
    assert max(n_rows) >= 99 and 1 in n_rows and 2 in n_rows and 3 in n_rows and 50 in n_rows


@pytest.mark.parametrize("k", (3, 4, 13))
def test_partitioned_sets(orc, k):
    for share in ("low", "high"):
        rows, pairs = M.partitioned_set(k, share)
        assert rows == M.dataset("partitioned_" + share, k)
        c, verdicts, _ = _check(orc, rows, k, "partitioned_" + share)
        assert set(pairs) == {(f, n) for f in range(4) for n in range(1, 10)}
        # the pairs are where the reads really start
        offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
        starts = {(int(offs[i]) % 4, len(r) - k + 1) for i, r in enumerate(rows[: 400]) if len(r) >= k and len(r) - k + 1 <= 9}
        assert set(pairs) <= starts
        keys, inst = M.keys_and_instances(rows, k)
        assert keys <= 0.25 * inst if share == "low" else keys >= 0.75 * inst
        assert c["tie-rescued"] >= 20 and c["tie-not"] >= 20


@pytest.mark.parametrize("n_ranks", (1, 2, 3))
@pytest.mark.parametrize("k", (3, 13))
def test_dealt_sets(orc, k, n_ranks):
    per_rank = M.dataset("dealt", k, n_ranks)
    rows = [r for part in per_rank for r in part]
    c, verdicts, _ = _check(orc, rows, k, f"dealt to {n_ranks}")
    assert c["tie-rescued"] >= 20 and c["tie-not"] >= 20
    if n_ranks > 1:
        # no copy sits with its probe: every rank holds long probes none of whose windows it holds as a one-window read
        for part in per_rank:
            copies = {M.canonical(r) for r in part if len(r) == k}
            alone = [r for r in part if len(r) - k + 1 > 16 and not copies & set(M._windows(r, k))]
            assert len(alone) >= 20 and len(alone) == sum(1 for r in part if len(r) - k + 1 > 16)
