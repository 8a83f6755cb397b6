"""The rescue pass of the first assembly iteration, restated from the reference's own words (graph/CreateMdbg.hpp:4514-4640), and
read sets whose k-min-mer counts are CHOSEN.  Plain Python, no GPU, nothing taken from the kernels' derivation of the rule.

The rule, per read: the abundance of every window (1 for a window seen once), Utils::compute_median of them (Commons.hpp:2972-2988: sort,
the middle one, for an even number the integer mean of the two middle ones), `median * 0.1f > 1` in float32 -> the read is left alone;
a read whose windows are all seen once is left alone too; otherwise every window of the read that was seen once is appended, in window
order, reads in read order.  The pass only runs when min_abundance <= 1 (graph/CreateMdbg.cpp:317-319).

How counts are chosen: a probe read of n + k - 1 distinct minimizers has n distinct windows; window w gets count c by adding c - 1
one-window reads equal to it."""
from __future__ import annotations

import functools
import random
from collections import Counter

import numpy as np

VERDICTS = ("no windows", "all ones", "rescued", "not", "tie-rescued", "tie-not")


def canonical(window) -> tuple:
    t = tuple(window)
    r = t[::-1]
    return t if t <= r else r


def _windows(row, k: int) -> list:
    return [canonical(row[i: i + k]) for i in range(len(row) - k + 1)]


def _left_alone(median: int) -> bool:
    """`median * 0.1f > 1`: u32 times float is a float32 product."""
    return bool(np.float32(median) * np.float32(0.1) > np.float32(1.0))


def rescued_rows(rows, k: int, min_abundance: int):
    """(rescued canonical windows in read order then window order, verdict per read, rescued rows per read).  A "tie" read is one with
    an even number of windows whose two middle counts, each taken as the median, would decide differently."""
    per_read = [_windows(r, k) for r in rows]
    count = Counter(w for ws in per_read for w in ws)
    out, verdicts, n_rows = [], [], []
    for ws in per_read:
        n = len(ws)
        if n == 0:
            verdicts.append("no windows"); n_rows.append(0)
            continue
        ab = sorted(count[w] for w in ws)
        if ab[-1] == 1:
            verdicts.append("all ones"); n_rows.append(0)
            continue
        if n % 2:
            median, tie = ab[n // 2], False
        else:
            median = (ab[n // 2 - 1] + ab[n // 2]) // 2
            tie = _left_alone(ab[n // 2 - 1]) != _left_alone(ab[n // 2])
        rescued = not _left_alone(median)
        verdicts.append(("tie-" if tie else "") + ("rescued" if rescued else "not"))
        mine = [w for w in ws if count[w] == 1] if rescued and min_abundance <= 1 else []
        out.extend(mine); n_rows.append(len(mine))
    if min_abundance > 1:
        assert not out
    return out, verdicts, n_rows


def census(rows, verdicts, k: int) -> dict:
    """Verdict -> number of reads, and the same for reads of more than 16 windows (more than one trip of a 16-lane group)."""
    c = {v: 0 for v in VERDICTS}
    c.update({v + " n>16": 0 for v in VERDICTS[2:]})
    for r, v in zip(rows, verdicts):
        c[v] += 1
        if v in VERDICTS[2:] and len(r) - k + 1 > 16:
            c[v + " n>16"] += 1
    return c


def keys_and_instances(rows, k: int) -> tuple[int, int]:
    ws = [w for r in rows for w in _windows(r, k)]
    return len(set(ws)), len(ws)


def to_arrays(rows) -> tuple[np.ndarray, np.ndarray]:
    mins = np.fromiter((v for r in rows for v in r), dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rows], dtype=np.int64)]).astype(np.uint64)
    return mins, offs


def canonical_rows(vecs: np.ndarray) -> list:
    return [canonical(v) for v in np.asarray(vecs).tolist()]


# ---- building ------------------------------------------------------------------------------------------------------------------------
class SetBuilder:
    """Reads in the order they are added; the one-window copies that make the counts are kept apart and go behind the reads (or are
    shuffled among them when rows() is asked to), so that read positions stay as chosen."""

    def __init__(self, k: int, first: int = 1000):
        self.k, self.nxt = k, first
        self.reads: list[list[int]] = []
        self.copies: list[list[int]] = []

    def fresh(self, m: int, descending: bool = False) -> list[int]:
        v = list(range(self.nxt, self.nxt + m))
        self.nxt += m + 1
        assert self.nxt < 1 << 32
        return v[::-1] if descending else v

    def probe(self, counts, descending: bool = False, palindrome_at: int | None = None) -> list[int]:
        """A read whose window w is seen counts[w] times in the set.  Ascending minimizers: every window is its own canonical form;
        descending: every stored vector is the reverse of the read's; palindrome_at: that window reads the same both ways (its
        neighbours stay distinct: they differ outside the part they share)."""
        k, n = self.k, len(counts)
        if n == 0:
            return self.add([])
        x = self.fresh(n + k - 1, descending)
        if palindrome_at is not None:
            p = palindrome_at
            for j in range(k // 2):
                x[p + k - 1 - j] = x[p + j]
        for w, c in enumerate(counts):
            assert c >= 1
            self.copies.extend([x[w: w + k]] * (c - 1))
        return self.add(x)

    def add(self, read) -> list[int]:
        self.reads.append(list(read))
        return self.reads[-1]

    def short(self, m: int) -> list[int]:
        """A read of m < k minimizers: no window."""
        assert m < self.k
        return self.add(self.fresh(m) if m else [])

    def all_ones(self, n: int) -> list[int]:
        return self.probe([1] * n)

    def self_contained(self, run_counts, n_weak: int) -> list[int]:
        """One read that makes its own counts: for each c of run_counts a run of k + c - 1 equal minimizers (c windows seen c times),
        k - 1 windows seen once where two runs meet, then n_weak fresh minimizers: as many more windows seen once."""
        x = []
        for c in run_counts:
            x += self.fresh(1) * (self.k + c - 1)
        return self.add(x + self.fresh(n_weak))

    def flat_offset(self) -> int:
        return sum(len(r) for r in self.reads)

    def rows(self, shuffle_seed: int | None = None) -> list[list[int]]:
        rows = self.reads + self.copies
        if shuffle_seed is not None:
            random.Random(shuffle_seed).shuffle(rows)
        return rows


def probe(counts, k: int, first: int = 1000) -> list[list[int]]:
    """The probe read of those counts and its copies, as rows."""
    b = SetBuilder(k, first)
    b.probe(counts)
    return b.rows()


# ---- §3a: the probe battery ----------------------------------------------------------------------------------------------------------
N_WINDOWS = (1, 2, 3, 4, 15, 16, 17, 18, 31, 32, 33, 34, 48, 64, 65, 100)
A_VALUES = (2, 9, 10)                           # largest count <= 10
B_VALUES = (11, 12, 20, 21, 22, 23)             # smallest count > 10; 21 - a and 22 - a are added: the median on 10 and on 11
HUGE = (254, 255, 256, 300)


def battery_counts(n: int, n_le: int, a: int, b: int, rng: random.Random, no_weak: bool, huge: bool) -> list[int]:
    """n counts, n_le of them <= 10 with the largest a, the others > 10 with the smallest b, at shuffled positions."""
    small = []
    if n_le:
        small = [a] + [(rng.randint(2, a) if no_weak or rng.random() < 0.25 else 1) for _ in range(n_le - 1)]
    big = []
    if n - n_le:
        big = [b] + [(rng.randint(b, 31) if rng.random() < 0.2 else b) for _ in range(n - n_le - 1)]
        if huge:
            for i in range(1, min(len(big), 5)):
                big[i] = HUGE[(i - 1) % 4]
    c = small + big
    rng.shuffle(c)
    return c


def battery(k: int, thin: int = 1, thin_ties_above: int = 1000, seed: int = 1, builder: SetBuilder | None = None) -> SetBuilder:
    """Every n of N_WINDOWS x {n/2 - 1, n/2, n/2 + 1, n} counts <= 10 x a x b.  thin > 1 keeps every thin-th probe (thin is coprime
    to the 20 (a, b) pairs of a cell, so every pair still occurs), but all the tie cells (n even, n/2 counts <= 10) up to
    thin_ties_above windows.  Every fifth probe has no count-1 window; one in 41 carries counts of 254 and above."""
    rng = random.Random(seed)
    sb = builder or SetBuilder(k)
    idx = 0
    for n in N_WINDOWS:
        sb.all_ones(n)
        for n_le in sorted({n // 2 - 1, n // 2, n // 2 + 1, n}):
            if n_le < 0:
                continue
            for a in A_VALUES:
                for b in sorted(set(B_VALUES) | {x for x in (21 - a, 22 - a) if x > 10}):
                    idx += 1
                    counts = battery_counts(n, n_le, a, b, rng, no_weak=idx % 5 == 0, huge=idx % 41 == 0)
                    tie_cell = n % 2 == 0 and n_le == n // 2 and n <= thin_ties_above
                    if tie_cell or idx % thin == 0:
                        sb.probe(counts, descending=idx % 2 == 1)
    return sb


# ---- §3b: read order chosen for a wave of four 16-lane groups ------------------------------------------------------------------------
def _tie4(a: int, b: int, c: int) -> list[int]:
    return [1, a, b, c]                          # four windows, two of them <= 10: rescued iff (a + min(b, c)) // 2 <= 10


def quadruples(sb: SetBuilder, reps: int) -> None:
    """Reads 4 i .. 4 i + 3 share a wave of the one-table kernels (the builder must hold a multiple of four reads)."""
    assert len(sb.reads) % 4 == 0
    for _ in range(reps):
        # tie-rescued, tie-not, rescued, not
        sb.probe(_tie4(10, 11, 30)); sb.probe(_tie4(10, 12, 12)); sb.probe([1, 2, 11, 1, 3]); sb.probe([11, 1, 12, 2, 25])
        # four ties with different (largest <= 10, smallest > 10)
        sb.probe(_tie4(2, 19, 19)); sb.probe(_tie4(2, 20, 300)); sb.probe(_tie4(9, 12, 21)); sb.probe(_tie4(9, 13, 13))
        # a tie beside a read shorter than k, an empty read and an all-ones read
        sb.short(sb.k - 1); sb.probe(_tie4(10, 12, 11)); sb.short(0); sb.all_ones(7)
        sb.all_ones(20); sb.short(1); sb.probe(_tie4(10, 12, 22)); sb.short(0)
        # a 100-window tie beside three 2-window reads: the loops' trip counts differ inside the wave
        sb.probe([2, 11]); sb.probe([1, 10] * 25 + [11, 12] * 25); sb.probe([1, 1]); sb.probe([1, 25])
        sb.probe([9, 13]); sb.probe([1, 3]); sb.probe([1, 25]); sb.probe([10, 1] * 25 + [12, 23] * 25)


def quadruple_set(k: int, reps: int = 50, more_reads_than: int = 0) -> SetBuilder:
    sb = SetBuilder(k)
    quadruples(sb, reps)
    while len(sb.reads) + len(sb.copies) <= more_reads_than:
        quadruples(sb, 10)
    return sb


def small_read_counts(k: int) -> SetBuilder:
    """Five reads that make their own counts, so that every prefix of the set is a set with the same counts: tie-not, tie-rescued,
    no windows, rescued, all ones."""
    sb = SetBuilder(k)
    sb.self_contained([22], 22)                  # 22 windows seen 22 times, 22 seen once: the median (1 + 22) // 2 = 11
    sb.self_contained([11], 11)                  # (1 + 11) // 2 = 6
    sb.short(k - 1)
    sb.self_contained([30], 40)
    sb.all_ones(5)
    return sb


# ---- §3c: the order of the rescued rows ----------------------------------------------------------------------------------------------
def weak_patterns(n: int) -> list[list[int]]:
    pats = [[0, 15], [15, 16, 17], [31, 32], list(range(n)), list(range(1, n)), list(range(0, n, 2)), [n - 1]]
    return [[p for p in pat if p < n] for pat in pats if any(p < n for p in pat)]


def row_order_set(k: int) -> SetBuilder:
    """Per pattern a read whose other windows are seen twice (rescued: the weak windows are its rows) and a twin whose other windows are
    seen 21 times (left alone unless the weak ones are the majority), alternately, so neighbours in a wave differ; ascending and
    descending minimizers alternate; then weak palindromic windows at 0, 15 and the end."""
    sb = SetBuilder(k)
    i = 0
    for n in (16, 17, 33, 100):
        for pat in weak_patterns(n):
            for other in (2, 21):
                sb.probe([1 if w in pat else other for w in range(n)], descending=i % 3 == 1)
                i += 1
    for n in (16, 17, 33):
        for p in (0, 15, n - 1):
            sb.probe([1 if w in (p, 3) else 2 for w in range(n)], palindrome_at=p)
            sb.probe([1 if w in (p, 3) else 21 for w in range(n)], palindrome_at=p, descending=True)
    return sb


# ---- §3d: flat offsets mod 4 and both fill values of the partitioned form's byte array -----------------------------------------------
def alignment_probes(sb: SetBuilder) -> list[tuple[int, int]]:
    """Probes of 1 .. 9 windows at every flat offset mod 4 (reads shorter than k in front move the offset); three count patterns each:
    only the last window weak, only the first, and a tie whose last window decides.  Returns the (offset mod 4, n) pairs made."""
    pairs = []
    for n in range(1, 10):
        for f in range(4):
            for variant in range(3):
                while sb.flat_offset() % 4 != f:
                    sb.short(min((f - sb.flat_offset()) % 4, sb.k - 1))
                if variant == 0:
                    counts = [2] * (n - 1) + [1]
                elif variant == 1:
                    counts = [1] + [2] * (n - 1)
                else:
                    counts = ([1, 10] * n)[: n // 2] + [30] * (n - n // 2 - 1) + [11 + (n + f) % 2]
                if n == 1:
                    counts = [(2, 1, 12)[variant]]
                pairs.append((sb.flat_offset() % 4, n))
                sb.probe(counts, descending=(n + f) % 2 == 1)
    return pairs


def partitioned_set(k: int, key_share: str) -> tuple[list[list[int]], list[tuple[int, int]]]:
    """The alignment probes in front, a thinned battery behind them, the copies last.  key_share "low": as it is (few distinct keys per
    instance); "high": all-ones reads of fresh minimizers are added until three quarters of the instances are distinct keys."""
    sb = SetBuilder(k)
    pairs = alignment_probes(sb)
    battery(k, thin=7, thin_ties_above=18, builder=sb)
    rows = sb.rows()
    if key_share == "high":
        keys, inst = keys_and_instances(rows, k)
        extra = max(0, 3 * inst - 4 * keys) + 64
        rows = rows + [sb.fresh(50 + k - 1) for _ in range(extra // 50 + 1)]
    return rows, pairs


# ---- §3e: dealt to ranks -------------------------------------------------------------------------------------------------------------
def dealt_set(k: int, n_ranks: int) -> list[list[list[int]]]:
    """The battery of this k, every probe on rank i mod n_ranks, its copies on the other ranks in turn: with more than one rank, every
    window of a probe is seen once by the rank that holds it."""
    sb = battery(k, *BATTERY_THIN[k])
    where = {tuple(r[w: w + k]): i % n_ranks for i, r in enumerate(sb.reads) for w in range(len(r) - k + 1)}
    per_rank = [[] for _ in range(n_ranks)]
    for i, r in enumerate(sb.reads):
        per_rank[i % n_ranks].append(r)
    for j, c in enumerate(sb.copies):
        home = where[tuple(c)]
        per_rank[(home + 1 + j % max(n_ranks - 1, 1)) % n_ranks if n_ranks > 1 else 0].append(c)
    return per_rank


# ---- the sets by name: what tests/test_rescue_model.py checks on the CPU is what tests/test_gpu_rescue_chosen_counts.py runs ---------
KS = (3, 4, 13, 33)
BATTERY_THIN = {3: (1, 1000), 4: (1, 1000), 13: (7, 34), 33: (11, 18)}      # k -> (thin, thin_ties_above): under 1.5 M minimizers


@functools.lru_cache(maxsize=None)
def dataset(name: str, k: int, arg: int = 0):
    """rows of the set (for "dealt": per rank)."""
    if name == "battery":
        thin, above = BATTERY_THIN[k]
        return battery(k, thin, above).rows(shuffle_seed=5)
    if name == "quadruples":
        return quadruple_set(k).rows()
    if name == "quadruples_sweeps":              # arg: the number of reads to exceed
        return quadruple_set(k, more_reads_than=arg).rows()
    if name == "prefix":                         # arg: the number of reads
        return small_read_counts(k).rows()[:arg]
    if name == "row_order":
        return row_order_set(k).rows()
    if name == "partitioned_low":
        return partitioned_set(k, "low")[0]
    if name == "partitioned_high":
        return partitioned_set(k, "high")[0]
    if name == "dealt":
        return dealt_set(k, arg)
    raise KeyError(name)
