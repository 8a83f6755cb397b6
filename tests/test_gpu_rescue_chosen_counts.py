"""The rescue pass (graph/CreateMdbg.hpp:4514-4640) on reads whose k-min-mer counts are CHOSEN (tests/rescue_model.py), in its three
forms, against the oracle, exactly: n_solid, the abundance records as a sorted multiset, the rescued rows vec[n_solid:] in the oracle's
order.  tests/test_rescue_model.py checks on the CPU that every set holds the cases named here.

  one table    csrc/kminmer.hip: slot_flag_kernel (2-bit count class), rescue_count_kernel (16 lanes a read, four reads a wave, the tie
               case behind a wave-wide __any), emit_rescued_kernel (row order from a slice of a wave-wide ballot)
  partitioned  csrc/partition.hip: rescue_count_p_kernel / emit_rescued_p_kernel over one byte per instance, read four at a time after an
               alignment prologue; the byte array starts as all 0 ("many") or all 1, by a sketch's estimate of keys against instances
  sharded      mdbg_shard_finish: one of the two over a rank's reads against the global counts

mdbg_first_pass_info does not say which fill value the partitioned form took, so the two sets of test_partitioned_offsets_and_fill_values
are built well to either side of its threshold (distinct keys at most a quarter, at least three quarters of the instances) and checked
by their results alone.

Out of scope: windows whose 128-bit hash has a zero word (the side-list slots s >= cap of count_class) would need a hash preimage.
GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from metamdbg_amd import formats
from tests import rescue_model as M
from tests.test_gpu_partition import PLANS, _options

pytestmark = pytest.mark.gpu

PART_MAX_K = 32
REPEATS, GROUPS = 4, 5                           # PLANS[4]: 8 x 256 slots must overflow and repeat; PLANS[5]: 1500 instances a group
FORMS = {"one_table": dict(first_pass_mode=1), "partitioned": dict(first_pass_mode=2), "partitioned_repeats": dict(first_pass_mode=2, **PLANS[REPEATS]),
         "partitioned_groups": dict(first_pass_mode=2, **PLANS[GROUPS])}


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


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def _arrays(name: str, k: int, arg: int = 0):
    return _frozen(*M.to_arrays(M.dataset(name, k, arg)))


@functools.lru_cache(maxsize=None)
def _expected(orc, name: str, k: int, arg: int, min_ab: int):
    """(n_solid, sorted abundance records, rescued rows in order) of the oracle, once per set."""
    mins, offs = _arrays(name, k, arg)
    exp = orc.kminmer_count_first(mins, offs, k, min_ab)
    return (exp["n_solid"],) + _frozen(formats.sorted_abundance_records(orc.table_abundance_records(exp)), exp["vecs"][exp["n_solid"]:].copy())


def _run(ctx, mins, offs, k: int, min_ab: int, form: str):
    _options(ctx, **FORMS[form])
    try:
        t = ctx.kminmer_count_first(ctx.minimizers_from_host(mins, offs), k, min_ab)
        info = ctx.first_pass_info()
    finally:
        _options(ctx)
    if form == "one_table" or k > PART_MAX_K:
        assert info["path"] == 1, info           # k > 32: the partitioned setting hands the input to the one-table pass
    else:
        assert info["path"] == 2, info
        if form == "partitioned_repeats":
            assert info["attempts"] > 1, info
        if form == "partitioned_groups":
            assert info["groups"] > 1, info
    return t


def _compare(rec, vec, got_n_solid: int, n_solid: int, records, rescued, min_ab: int):
    assert got_n_solid == n_solid
    assert len(rec) - n_solid == len(rescued), f"{len(rec) - n_solid} rescued rows for the oracle's {len(rescued)}"
    assert np.array_equal(formats.sorted_abundance_records(rec), records)
    assert (rec[:n_solid]["abundance"] > 1).all() and (rec[n_solid:]["abundance"] == 1).all()
    if min_ab > 1:
        assert len(rec) == n_solid and len(rescued) == 0         # no row of abundance 1 at all
    assert vec[n_solid:].shape == rescued.shape
    bad = np.flatnonzero((vec[n_solid:] != rescued).any(axis=1))
    assert len(bad) == 0, f"{len(bad)} of {len(rescued)} rescued rows differ, the first at {bad[0]}: {vec[n_solid + bad[0]]} for {rescued[bad[0]]}"


def _check(ctx, orc, name: str, k: int, min_ab: int, form: str, arg: int = 0):
    mins, offs = _arrays(name, k, arg)
    n_solid, records, rescued = _expected(orc, name, k, arg, min_ab)
    t = _run(ctx, mins, offs, k, min_ab, form)
    got_n_solid = t.info()["n_solid"]
    rec, vec = t.to_host()
    t.free()
    _compare(rec, vec, got_n_solid, n_solid, records, rescued, min_ab)


# ---- a. the probe battery --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("min_ab", [0, 1, 2])
@pytest.mark.parametrize("k", M.KS)
def test_probe_battery(ctx, orc, k, min_ab, form):
    """Probes of 1 .. 100 windows with n/2 - 1, n/2, n/2 + 1 or n counts <= 10, the largest of them 2, 9 or 10, the smallest count
    above from 11 to 23 so that the median of a tie falls on 10 and on 11; counts up to 300; probes without a count-1 window; all-ones
    probes.  k = 13 is the generic window hash, k = 33 more than the partitioned form takes."""
    _check(ctx, orc, "battery", k, min_ab, form)


# ---- b. read order chosen for the one-table wave ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one_table", "partitioned"])
@pytest.mark.parametrize("k", [3, 4])
def test_hand_laid_waves(ctx, orc, k, form):
    """Reads 4 i .. 4 i + 3 share a wave of rescue_count_kernel and emit_rescued_kernel: tie-rescued, tie-not, rescued, not; four ties with
    different (largest <= 10, smallest > 10); a tie beside a short, an empty and an all-ones read; a 100-window tie beside three 2-window
    reads.  Fifty times over with fresh minimizers."""
    _check(ctx, orc, "quadruples", k, 0, form)


@pytest.mark.parametrize("form", ["one_table", "partitioned"])
@pytest.mark.parametrize("n_reads", [1, 2, 3, 5])
@pytest.mark.parametrize("k", [3, 4, 33])
def test_a_partly_live_last_wave(ctx, orc, k, n_reads, form):
    """One, two, three and five reads that make their own counts (runs of one minimizer): tie-not, tie-rescued, no windows, rescued, all
    ones."""
    _check(ctx, orc, "prefix", k, 0, form, n_reads)


@pytest.mark.parametrize("form", ["one_table", "partitioned"])
def test_more_reads_than_two_sweeps_of_the_capped_grid(ctx, orc, form):
    """rescue_count_kernel and emit_rescued_kernel run at most n_cu x 16 blocks of 16 groups: with more than twice as many reads the r0 loop
    makes several trips, the last with dead groups."""
    n_cu = ctx.device_info()["n_cu"]
    floor = 2 * n_cu * 16 * 16
    _, offs = _arrays("quadruples_sweeps", 3, floor)
    n_reads = len(offs) - 1
    assert n_reads > floor and n_reads % (n_cu * 16 * 16) != 0
    _check(ctx, orc, "quadruples_sweeps", 3, 0, form, floor)


# ---- c. the order of the rescued rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one_table", "partitioned"])
@pytest.mark.parametrize("k", [3, 4, 13])
def test_row_order(ctx, orc, k, form):
    """Reads of 16, 17, 33 and 100 windows with the count-1 windows at {0, 15}, {15, 16, 17}, {31, 32}, everywhere (an all-ones read: no
    row), everywhere but 0, every second position, the last position; each beside a twin that is left alone; weak palindromic windows and
    reads whose stored vectors are reversed."""
    _check(ctx, orc, "row_order", k, 0, form)


# ---- d. the partitioned form's byte array ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share,form", [(s, f) for s in ("low", "high") for f in FORMS if (s, f) != ("high", "partitioned_repeats")])
@pytest.mark.parametrize("k", [3, 4, 13])
def test_partitioned_offsets_and_fill_values(ctx, orc, k, share, form):
    """Probes of 1 .. 9 windows at every flat offset mod 4 (prologue, 4-byte loop and tail of rescue_count_p_kernel in every split), in a
    set with few distinct keys per instance (the array starts as "many") and in one with many (it starts as 1).  The plan that repeats
    is left out of the second: its 172 538 keys are more than the 512 x 256 slots of its fourth and last attempt hold."""
    _check(ctx, orc, "partitioned_" + share, k, 0, form)


# ---- e. sharded ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dealt(orc, k: int, n_ranks: int):
    """Per rank (mins, offs, its rescued rows in its read order); the whole set's (n_solid, sorted records)."""
    per_rank = M.dataset("dealt", k, n_ranks)
    rows = [r for part in per_rank for r in part]
    mins, offs = M.to_arrays(rows)
    exp = orc.kminmer_count_first(mins, offs, k, 0)
    rescued = exp["vecs"][exp["n_solid"]:]
    n_rows = M.rescued_rows(rows, k, 0)[2]       # rows per read: which of the oracle's rescued rows are whose
    assert sum(n_rows) == len(rescued)
    ranks, read0, row0 = [], 0, 0
    for part in per_rank:
        n = sum(n_rows[read0: read0 + len(part)])
        ranks.append(_frozen(*M.to_arrays(part), rescued[row0: row0 + n].copy()))
        read0 += len(part); row0 += n
    return ranks, exp["n_solid"], _frozen(formats.sorted_abundance_records(orc.table_abundance_records(exp)))[0]


@pytest.mark.parametrize("form", ["one_table", "partitioned"])
@pytest.mark.parametrize("n_ranks", [1, 2, 3])
@pytest.mark.parametrize("k", [3, 13])
def test_sharded_finish(ctx, orc, k, n_ranks, form):
    """The battery dealt so that a probe and its one-window copies sit on different ranks: every window of a probe is count-1 locally and
    has its chosen count globally.  mdbg_shard_begin, the two exchanges through host copies (as test_sharded_first_pass_on_one_gpu),
    mdbg_shard_finish: every rank's rescued rows are the whole set's rescued rows of its own reads, in its read order; the union of the
    solid rows is the whole set's."""
    from tests.test_gpu_shard_chosen_keys import _Hip
    hip = _Hip()
    ranks, n_solid, records = _dealt(orc, k, n_ranks)
    _options(ctx, **FORMS[form])
    bufs, tables, sh = [], [], []
    reads = [ctx.minimizers_from_host(mins, offs) for mins, offs, _ in ranks]     # mdbg_shard_begin: alive until mdbg_shard_free
    try:
        for part in reads:
            sh.append(ctx.shard_begin(part, k, n_ranks))
            if form == "partitioned":
                assert ctx.first_pass_info()["path"] == 2
        rw = sh[0].row_words
        sent = [hip.to_host(s.d_rows, (s.n_rows, rw)) for s in sh]
        per_owner = [[] for _ in range(n_ranks)]
        for r in range(n_ranks):
            o = 0
            for dst in range(n_ranks):
                c = int(sh[r].counts[dst])
                per_owner[dst].append(sent[r][o: o + c]); o += c
        replies = []
        for dst in range(n_ranks):
            rows = np.ascontiguousarray(np.concatenate(per_owner[dst]))
            bufs.append(hip.to_device(rows))
            replies.append(hip.to_host(sh[dst].reduce(bufs[-1].value, len(rows)), (len(rows),)))
        for r in range(n_ranks):
            glob = []
            for dst in range(n_ranks):
                o = sum(int(sh[src].counts[dst]) for src in range(r))
                glob.append(replies[dst][o: o + int(sh[r].counts[dst])])
            glob = np.ascontiguousarray(np.concatenate(glob))
            assert len(glob) == sh[r].n_rows
            bufs.append(hip.to_device(glob))
            tables.append(sh[r].finish(bufs[-1].value, 0))
        got = [(t.info()["n_solid"],) + t.to_host() for t in tables]
    finally:
        _options(ctx)
        for s in sh:
            s.free()
        for b in bufs:
            hip.free(b)
        for part in reads:
            part.free()
    for (ns, rec, vec), (_, _, rescued) in zip(got, ranks):
        assert (rec[:ns]["abundance"] > 1).all() and (rec[ns:]["abundance"] == 1).all()
        assert vec[ns:].shape == rescued.shape and np.array_equal(vec[ns:], rescued)
    assert sum(g[0] for g in got) == n_solid
    assert np.array_equal(formats.sorted_abundance_records(np.concatenate([g[1] for g in got])), records)
