""""table_wave_priority" (raise_wave_priority, csrc/common.hpp): the wave priority of the kernels a step launches outside
the scan -- the purge's, the partitioned first pass's, the prefix scans' -- changes when their instructions issue, never what they
compute.  Purge (4, 100) plus the first pass at k = 4 at levels 0, 1 and 3, with the four-wave and the eight-wave split kernels and
with the options bench.py gives a context that shares its device: the purge's output against the oracle value for value, the table's
records and vectors against the oracle's (sorted: a bucket's rows come out in the order its waves reach them), and the levels against
each other.  mdbg_first_pass_form's third word says which level the last such kernel was launched with.
Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import threading

import numpy as np
import pytest

from metamdbg_amd import synth

pytestmark = pytest.mark.gpu

K = 4
FIRST_K, LAST_K = 4, 100
LEVELS = (0, 1, 3)
# the options bench.py gives every context that shares its device (its shared_opts)
BENCH_SHARED = {"scan_lds_reserve": 28672, "partition_tile": 2048, "partition_slot_list": 0, "partition_lds_slots": 1024}
FORMS = {"threads256": dict(partition_threads=256), "threads512": dict(partition_threads=512), "bench_shared": dict(BENCH_SHARED)}
OPTION_NAMES = ("partition_lds_slots", "partition_threads", "partition_tile", "scan_lds_reserve")
SHARED_DEFAULT = 1          # TABLE_WAVE_PRIORITY_SHARED (csrc/common.hpp): the level a context that shares its device takes by itself


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    c.set_option("first_pass_mode", 2)
    yield c
    c.close()


def _csr(lists):
    offs = np.zeros(len(lists) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in lists], out=offs[1:])
    mins = np.concatenate([np.asarray(x, dtype=np.uint32) for x in lists] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return mins, offs


def _clean_reads(rng, n_instances, genome_len=400):
    """Reads cut from a few strictly increasing sequences: no palindromic window anywhere (the purge copies them), windows shared between
    reads (solid keys), exactly n_instances windows of K in all; an empty read and reads shorter than K among them."""
    genomes = [np.cumsum(rng.integers(1, 5, genome_len)).astype(np.uint32) + 1000 * g for g in range(3)]
    lists, left = [], n_instances
    while left > 0:
        inst = int(min(left, rng.integers(1, 57)))
        g = genomes[int(rng.integers(0, len(genomes)))]
        s = int(rng.integers(0, genome_len - (inst + K - 1) + 1))
        lists.append(g[s: s + inst + K - 1])
        left -= inst
    lists += [np.zeros(0, np.uint32), genomes[0][:2], genomes[1][:K - 1]]
    assert sum(max(len(x) - (K - 1), 0) for x in lists) == n_instances
    return lists


def _three_reads(rng):
    g = np.cumsum(rng.integers(1, 5, 40)).astype(np.uint32)
    return [g[:12], g[3:20], g[:12]]


def _short_and_empty(rng):
    """An empty read and a read shorter than K between reads that have windows."""
    g = np.cumsum(rng.integers(1, 5, 60)).astype(np.uint32)
    return [g[:9], np.zeros(0, np.uint32), g[:K - 1], g[2:30], g[:2], g[:9], np.zeros(0, np.uint32)]


def _palindromes(rng):
    """Planted palindromic windows of lengths 4 .. 7 in otherwise clean reads: purge_fix_kernel drops minimizers of every second read."""
    lists = []
    for r in range(60):
        g = (np.cumsum(rng.integers(1, 5, int(rng.integers(8, 120)))) + 5000).astype(np.uint32)
        if r % 2 == 0:
            length = 4 + r % 4
            half = g[: (length + 1) // 2]
            pal = np.concatenate([half, half[::-1][length % 2:]])
            at = int(rng.integers(0, len(g)))
            g = np.concatenate([g[:at], pal, g[at:]]).astype(np.uint32)
        lists.append(g)
    return lists + lists[:20]


def _rare(rng):
    """Reads whose k-min-mers are all rare: two copies of a read and a third that shares half of it -- the shared windows are counted
    three times, the third read's own once, so that read is rescued and its count-1 windows become rows; beside them solid filler."""
    lists = []
    for r in range(12):
        g = (np.cumsum(rng.integers(1, 5, 40)) + 100000 * (r + 1)).astype(np.uint32)
        own = (np.cumsum(rng.integers(1, 5, 14)) + 100000 * (r + 1) + 50000).astype(np.uint32)
        lists += [g, g, np.concatenate([g[:20], own])]
    return lists + _clean_reads(rng, 500)


# name -> the reads in minimizer space.  Instance counts around the split kernels' tiles of 1024 (four waves), 2048 (bench's) and 4096.
def _make(name, rng):
    if name.startswith("tile"):
        return _clean_reads(rng, int(name[4:]))
    return {"3reads": _three_reads, "short_and_empty": _short_and_empty, "palindromes": _palindromes, "rare": _rare}[name](rng)


BATCHES = ["3reads", "short_and_empty", "palindromes", "rare"] + [f"tile{t + d}" for t in (1024, 2048, 4096) for d in (-1, 0, 1)]
_cache: dict = {}


def _sorted_table(rec, vec):
    order = np.lexsort((rec["abundance"], rec["lo"], rec["hi"]))
    return rec[order], vec[order]


def _reference(orc, name):
    """The batch, the oracle's purge of it and the oracle's table of the purged reads: made once, shared, never written to."""
    if name not in _cache:
        lists = _make(name, np.random.default_rng(7000 + BATCHES.index(name)))
        mins, offs = _csr(lists)
        pmins, poffs = _csr([orc.purge_palindrome(x, FIRST_K, LAST_K) for x in lists])
        exp = orc.kminmer_count_first(pmins, poffs, K, 0)
        rec, vec = _sorted_table(orc.table_abundance_records(exp), exp["vecs"])
        for a in (mins, offs, pmins, poffs, rec, vec):
            a.setflags(write=False)
        _cache[name] = dict(mins=mins, offs=offs, pmins=pmins, poffs=poffs, rec=rec, vec=vec, n_solid=exp["n_solid"], n=exp["n"])
    return _cache[name]


def _set(ctx, **kw):
    for name in OPTION_NAMES:
        ctx.set_option(name, kw.get(name, 0))
    ctx.set_option("partition_slot_list", kw.get("partition_slot_list", 1))


def _step(ctx, mins, offs, level, **options):
    """Purge and first pass at one level; the host arrays and the level each call reports."""
    _set(ctx, **options)
    ctx.set_option("table_wave_priority", level)
    try:
        purged = ctx.purge_palindromes(ctx.minimizers_from_host(mins, offs), FIRST_K, LAST_K)
        ran_purge = ctx.table_wave_priority()
        p = purged.to_host(full=False)
        t = ctx.kminmer_count_first(purged, K, 0)
        info, ran_pass = ctx.first_pass_info(), ctx.table_wave_priority()
    finally:
        _set(ctx)
        ctx.set_option("table_wave_priority", 0)
    rec, vec = _sorted_table(*t.to_host())
    return dict(pmins=p["minimizers"], poffs=p["offsets"], rec=rec, vec=vec, n_solid=t.info()["n_solid"], info=info, ran=(ran_purge, ran_pass))


def _assert_step(got, ref, what):
    assert np.array_equal(got["poffs"], ref["poffs"]) and np.array_equal(got["pmins"], ref["pmins"]), f"{what}: purge"
    assert got["info"]["path"] == 2 or len(ref["pmins"]) < K, (what, got["info"])
    assert got["n_solid"] == ref["n_solid"] and len(got["rec"]) == ref["n"], (what, got["n_solid"], ref["n_solid"], len(got["rec"]), ref["n"])
    assert np.array_equal(got["rec"], ref["rec"]), f"{what}: records"
    assert np.array_equal(got["vec"], ref["vec"]), f"{what}: vectors"


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("batch", BATCHES)
def test_levels_agree_with_the_oracle_and_each_other(ctx, orc, batch, form):
    ref = _reference(orc, batch)
    if batch == "palindromes":
        assert len(ref["pmins"]) < len(ref["mins"])             # the purge drops something
    if batch == "rare":
        assert ref["n"] > ref["n_solid"]                        # rescue rows are written
    if batch.startswith("tile"):
        assert len(ref["pmins"]) == len(ref["mins"])            # the tile's count is what the first pass sees
    got = {}
    for level in LEVELS:
        got[level] = _step(ctx, ref["mins"], ref["offs"], level, **FORMS[form])
        assert got[level]["ran"] == (level, level), (level, got[level]["ran"])
        _assert_step(got[level], ref, f"{batch}, {form}, level {level}")
        if batch.startswith("tile"):
            assert got[level]["info"]["instances"] == int(batch[4:]), got[level]["info"]
    for level in LEVELS[1:]:
        for name in ("pmins", "poffs", "rec", "vec"):
            assert np.array_equal(got[level][name], got[0][name]), (level, name)
        assert got[level]["n_solid"] == got[0]["n_solid"]


def test_option_clamps_like_scan_wave_priority_and_reports_what_ran(ctx):
    mins, offs = _csr(_three_reads(np.random.default_rng(1)))
    try:
        for value, level in ((-1, 0), (0, 0), (3, 3), (7, 3), (1, 1), (2, 2)):
            ctx.set_option("table_wave_priority", value)
            ctx.set_option("scan_wave_priority", value)         # the same clamp: both accept any value
            ctx.purge_palindromes(ctx.minimizers_from_host(mins, offs), FIRST_K, LAST_K)
            assert ctx.table_wave_priority() == level, (value, ctx.table_wave_priority())
            ctx.kminmer_count_first(ctx.minimizers_from_host(mins, offs), K, 0)
            assert ctx.table_wave_priority() == level, (value, ctx.table_wave_priority())
    finally:
        ctx.set_option("table_wave_priority", 0)
        ctx.set_option("scan_wave_priority", 0)


def test_default_level_of_a_fresh_context():
    """Where the option was never set: SHARED_DEFAULT in a context that shares its device ("scan_lds_reserve" > 0), 0 in every other; the option
    overrides both, 0 included."""
    from metamdbg_amd import capi
    mins, offs = _csr(_three_reads(np.random.default_rng(2)))
    c = capi.Context(0)
    try:
        c.purge_palindromes(c.minimizers_from_host(mins, offs), FIRST_K, LAST_K)
        assert c.table_wave_priority() == 0
        c.set_option("scan_lds_reserve", 28672)
        c.purge_palindromes(c.minimizers_from_host(mins, offs), FIRST_K, LAST_K)
        assert c.table_wave_priority() == SHARED_DEFAULT
        c.set_option("table_wave_priority", 0)
        c.purge_palindromes(c.minimizers_from_host(mins, offs), FIRST_K, LAST_K)
        assert c.table_wave_priority() == 0
        c.set_option("table_wave_priority", 2)
        c.set_option("scan_lds_reserve", 0)
        c.purge_palindromes(c.minimizers_from_host(mins, offs), FIRST_K, LAST_K)
        assert c.table_wave_priority() == 2
    finally:
        c.close()


# ---- two contexts on one device: A scans (persistent launch), B purges and counts at level 3 on a thread of its own -------------------
def _ascii(codes) -> bytes:
    return bytes(synth.CODE2ASCII[np.asarray(codes, dtype=np.int64)])


def _read(rng, n) -> bytes:
    c = np.cumsum(np.concatenate([rng.integers(0, 4, 1), rng.integers(1, 4, n - 1)])) % 4
    return _ascii(np.repeat(c, rng.choice([1, 1, 2, 3], len(c))))


def test_first_pass_at_level_3_beside_another_contexts_persistent_scan(orc):
    """3000 reads of 500 - 5000 bases, not the 100 000 of 10 kb the case may have at most: the oracle scans every read on one host thread, and
    what is checked -- both contexts' results while their kernels share the device -- does not grow with the batch."""
    from metamdbg_amd import capi
    rng = np.random.default_rng(515)
    genome = [_read(rng, 3000) for _ in range(40)]
    seqs = []
    for _ in range(3000):                                       # reads of 500 - 5000 bases cut from a few sequences: windows repeat
        g = genome[int(rng.integers(0, len(genome)))]
        n = int(rng.integers(500, min(5000, len(g))))
        s = int(rng.integers(0, len(g) - n + 1))
        seqs.append(g[s: s + n])
    recs = [orc.read_selection(s, None, K=15, density=0.005, hpc=True) for s in seqs]
    e_mins, e_offs = _csr([r["minimizers"] for r in recs])
    lists = [np.asarray(r["minimizers"], np.uint32) for r in recs]
    pmins, poffs = _csr([orc.purge_palindrome(x, FIRST_K, LAST_K) for x in lists])
    exp = orc.kminmer_count_first(pmins, poffs, K, 0)
    ref = dict(pmins=pmins, poffs=poffs, n_solid=exp["n_solid"], n=exp["n"])
    ref["rec"], ref["vec"] = _sorted_table(orc.table_abundance_records(exp), exp["vecs"])
    rounds = 5
    a, b = capi.Context(0), capi.Context(0)
    scanned, counted, errors = [], [], []

    def scans():
        try:
            for name, value in dict(scan_prefilter=1, scan_persistent=1, **BENCH_SHARED).items():
                a.set_option(name, value)
            for _ in range(rounds):
                reads = a.reads_from_ascii(seqs)
                m = a.scan(reads, K=15, density=0.005, hpc=True, apply_read_filters=True)
                scanned.append((m.to_host(full=False), a.scan_persistent_info()))
                m.free()
                reads.free()
        except Exception as exc:                                # noqa: BLE001 -- reported by the test's own thread
            errors.append(exc)

    def passes():
        try:
            b.set_option("first_pass_mode", 2)
            for _ in range(rounds):
                counted.append(_step(b, e_mins, e_offs, 3, **BENCH_SHARED))
        except Exception as exc:                                # noqa: BLE001
            errors.append(exc)

    try:
        threads = [threading.Thread(target=scans), threading.Thread(target=passes)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert len(scanned) == rounds and len(counted) == rounds
        for h, info in scanned:
            assert info["form"] == "persistent", info
            assert np.array_equal(h["offsets"], e_offs) and np.array_equal(h["minimizers"], e_mins)
        for i, got in enumerate(counted):
            assert got["ran"] == (3, 3), got["ran"]
            _assert_step(got, ref, f"pass {i} beside the scan")
    finally:
        a.close()
        b.close()
