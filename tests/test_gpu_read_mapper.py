"""mdbg_map_index_build / mdbg_map_anchors / mdbg_map_chains (csrc/mapper.hip, mapper_dev.hpp) on the device.

Against the REFERENCE: tests/golden/read_mapper holds what ReadMapper.hpp's own ReadFunctor, sortParallel, createLookupTable and chainAnchors
computed for seeded reads at bands 62, 5 and 100 (mapper_ref.cpp; tests/test_read_mapper_model.py holds the numpy model against the same
files).  Index (per pair, as sorted rows: the reference's order inside a pair is whatever its sort left), anchors with min_anchors 1 and
3, and every chain field and match list are compared for equality.

Against the model (tests/mapper_model.py), on inputs the fixture does not have: query slices, global read numbers, a pair that 5 000 index
entries share, chains of 1 000 and 1 500 anchors (below and above the 1 024 anchors whose scores a wave keeps in LDS), pairs of exactly
band, band + 1 and 64 n +- 1 anchors, a grid of anchors that takes three trips of the band, a pair too long to chain, empty inputs.

Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

from tests import mapper_model as mm

pytestmark = pytest.mark.gpu

CONFIGS = [(c["name"], c["band"]) for c in mm.fixture_manifest()["configs"]]


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def upload(ctx, reads):
    """reads: (minimizers, offsets, positions)"""
    return ctx.minimizers_with_positions(*reads)


def pack(reads: list) -> tuple:
    """[(minimizers, positions), ...] -> (minimizers, offsets, positions)"""
    off = np.concatenate([[0], np.cumsum([len(m) for m, _ in reads])]).astype(np.uint64)
    cat = lambda k: np.concatenate([np.asarray(r[k], np.uint32) for r in reads]) if reads else np.zeros(0, np.uint32)
    return cat(0), off, cat(1)


def device(ctx, chunk, queries, band, min_anchors=1, chunk_first=0, query_first=0, query_begin=0, query_end=0) -> tuple:
    """(index rows, index info, anchors, chains, chain info) as the library computes them"""
    cm = upload(ctx, chunk)
    qm = cm if queries is chunk else upload(ctx, queries)
    ix = ctx.map_index_build(cm, chunk_first)
    an = ctx.map_anchors(ix, qm, query_first, min_anchors, query_begin, query_end, band)
    ch = ctx.map_chains(an, band)
    out = ix.to_host(), ix.info(), an.to_host(), ch.to_host(), ch.info()
    assert an.info() == dict(n_queries=len(out[2]["pair_offsets"]) - 1, n_pairs=len(out[2]["pair_ref_read"]), n_anchors=len(out[2]["ref_read"]),
                             longest_pair=int(np.diff(out[2]["anchor_offsets"].astype(np.int64)).max()) if len(out[2]["pair_ref_read"]) else 0)
    for h in (ch, an, ix, qm, cm):
        h.free()
    return out


def model(chunk, queries, band, min_anchors=1, chunk_first=0, query_first=0, query_begin=0, query_end=0) -> tuple:
    ix = mm.build_index(*chunk, first_read=chunk_first)
    an = mm.anchors(ix, *queries, query_first_read=query_first, min_anchors=min_anchors, query_begin=query_begin, query_end=query_end)
    return ix, an, mm.chains(an, band)


def same_as_model(ctx, chunk, queries, band, **kw) -> tuple:
    rows, info, an, ch, chinfo = device(ctx, chunk, queries, band, **kw)
    mix, man, mch = model(chunk, queries, band, **kw)
    for k in ("pair", "read", "position", "index", "reversed"):
        assert np.array_equal(rows[k], mix[k]), k
    assert {k: info[k] for k in ("n_entries", "n_pairs", "longest_run")} == mm.index_info(mix)
    mm.same(an, man)
    mm.same(ch, mch)
    assert chinfo["n_chains"] == int((mch["chains"]["flags"] == mm.CHAIN_FOUND).sum()) and chinfo["n_matches"] == len(mch["matches"])
    return an, ch


# ---- the reference's fixture ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=CONFIGS, ids=[c[0] for c in CONFIGS])
def case(request, ctx):
    name, band = request.param
    d = mm.load_fixture(name)
    reads = (d["minimizers"], d["read_offsets"], d["positions"])
    return dict(name=name, band=band, d=d, reads=reads, got={m: device(ctx, reads, reads, band, min_anchors=m) for m in (1, 3)})


def test_index_against_the_reference(case):
    d = case["d"]
    rows, info = case["got"][1][0], case["got"][1][1]
    ref = np.lexsort((d["index_index"], d["index_read"], d["index_pair"]))        # per pair as sorted rows; the device's order inside a pair is (read, index)
    for mine, theirs in (("pair", "index_pair"), ("read", "index_read"), ("position", "index_position"), ("index", "index_index"), ("reversed", "index_reversed")):
        assert np.array_equal(rows[mine], d[theirs][ref]), mine
    runs = np.diff(np.flatnonzero(np.concatenate([[True], d["index_pair"][1:] != d["index_pair"][:-1], [True]])))
    assert info == dict(n_entries=len(d["index_pair"]), n_pairs=len(runs), longest_run=int(runs.max()), n_reads=len(d["read_offsets"]) - 1)


@pytest.mark.parametrize("min_anchors", [1, 3])
def test_anchors_against_the_reference(case, min_anchors):
    mm.same(case["got"][min_anchors][2], mm.fixture_anchors(case["d"], min_anchors))


@pytest.mark.parametrize("min_anchors", [1, 3])
def test_chains_against_the_reference(case, min_anchors):
    want = mm.fixture_chains(case["d"], min_anchors)
    mm.same(case["got"][min_anchors][3], want)
    assert case["got"][min_anchors][4]["n_chains"] == int((want["chains"]["flags"] == mm.CHAIN_FOUND).sum()) > 100


@pytest.mark.parametrize("step", [1, 7, 0])
def test_query_slices_concatenate_to_the_whole(ctx, step):
    d = mm.load_fixture("band62")
    reads = (d["minimizers"], d["read_offsets"], d["positions"])
    n = len(d["read_offsets"]) - 1
    m = upload(ctx, reads)
    ix = ctx.map_index_build(m)
    parts_a, parts_c = [], []
    for b in range(0, n, step or n):
        an = ctx.map_anchors(ix, m, 0, 3, b, min(b + (step or n), n), 62)
        ch = ctx.map_chains(an, 62)
        parts_a.append(an.to_host()); parts_c.append(ch.to_host())
        an.free(); ch.free()

    def join(parts, offsets):
        out = {}
        for k in parts[0]:
            if k in offsets:          # a CSR offset array: rebased on what came before
                base, rows = 0, [np.zeros(1, np.uint64)]
                for p in parts:
                    rows.append(p[k][1:] + np.uint64(base))
                    base += int(p[k][-1])
                out[k] = np.concatenate(rows)
            else:
                out[k] = np.concatenate([p[k] for p in parts])
        return out

    mm.same(join(parts_a, ("pair_offsets", "anchor_offsets")), mm.fixture_anchors(d, 3))
    mm.same(join(parts_c, ("pair_offsets", "match_offsets")), mm.fixture_chains(d, 3))
    ix.free(); m.free()


# ---- against the model ---------------------------------------------------------------------------------------------------------------------
def test_self_hits_follow_the_global_read_numbers(ctx):
    d = mm.load_fixture("band5")
    sub = lambda a, b: (d["minimizers"][int(d["read_offsets"][a]):int(d["read_offsets"][b])], d["read_offsets"][a:b + 1] - d["read_offsets"][a],
                        d["positions"][int(d["read_offsets"][a]):int(d["read_offsets"][b])])
    chunk, queries = sub(0, 60), sub(30, 90)
    # the same reads under the same numbers: queries 1030 .. 1059 are chunk reads 1030 .. 1059 and leave their own entries out
    an, _ = same_as_model(ctx, chunk, queries, 5, chunk_first=1000, query_first=1030)
    assert an["pair_ref_read"].min() >= 1000
    own = [int(q) + 1030 in an["pair_ref_read"][int(an["pair_offsets"][q]):int(an["pair_offsets"][q + 1])].tolist() for q in range(30)]
    assert not any(own)
    # under other numbers every read meets itself
    an, _ = same_as_model(ctx, chunk, queries, 5, chunk_first=1000, query_first=0)
    lens = np.diff(queries[1].astype(np.int64))
    met = [1030 + q in an["pair_ref_read"][int(an["pair_offsets"][q]):int(an["pair_offsets"][q + 1])].tolist() for q in range(30) if lens[q] >= 10]
    assert met and all(met)
    same_as_model(ctx, chunk, queries, 5, chunk_first=0xFFFFFFFF - 59, query_first=0xFFFFFFFF - 59 - 30, min_anchors=3)


def test_one_pair_5000_times_in_the_chunk(ctx):
    """50 reads of 100 windows of one pair; one query window hits all 5 000 entries: the anchors are dealt to the waves, not the windows."""
    a, b = 77, 1234567
    chunk = [(np.tile([a, b], 51)[:101], 100 + 40 * np.arange(101)) for _ in range(50)]
    rng = np.random.default_rng(3)
    q = np.concatenate([rng.integers(1 << 20, 1 << 30, 8), [a, b], rng.integers(1 << 20, 1 << 30, 6)])
    queries = [(q, 500 + 37 * np.arange(len(q))), (rng.integers(1 << 20, 1 << 30, 12), 10 * np.arange(1, 13))]
    an, ch = same_as_model(ctx, pack(chunk), pack(queries), 62, query_first=1000)      # (other reads than the chunk's: no entry is the query's own)
    assert len(an["ref_read"]) == 5000 and list(an["pair_offsets"]) == [0, 50, 50] and set(an["query_index"].tolist()) == {8}
    assert not ch["chains"]["flags"].any()              # one query position: nothing can follow anything


@pytest.mark.parametrize("n_anchors", [1000, 1500])
def test_a_long_chain(ctx, n_anchors):
    """Two copies of one read: a pair of n anchors in one chain -- 1 000 in a wave's LDS, 1 500 in the pooled global buffer."""
    rng = np.random.default_rng(n_anchors)
    m = rng.permutation(1 << 20)[:n_anchors + 1].astype(np.uint32) + 1
    pos = np.cumsum(rng.integers(20, 60, n_anchors + 1))
    jitter = pos + np.cumsum(rng.integers(-1, 2, n_anchors + 1)) + 5000
    reads = pack([(m, pos), (m, jitter), (m[::-1], pos[-1] + 50 - pos[::-1])])
    an, ch = same_as_model(ctx, reads, reads, 62)
    assert list(np.diff(an["anchor_offsets"].astype(np.int64))) == [n_anchors] * 6
    rows = ch["chains"]
    assert (rows["flags"] == mm.CHAIN_FOUND).all() and (rows["n_matches"] > 0.9 * n_anchors).all() and set(rows["query_reversed"].tolist()) == {0, 1}


@pytest.mark.parametrize("band", [1, 62, 64, 65, 130])
def test_pair_sizes_at_the_band_and_at_the_wave(ctx, band):
    """Pairs of exactly band, band + 1 and 64 n +- 1 anchors: one read and its jittered copy each."""
    rng = np.random.default_rng(band)
    reads = []
    for n in sorted({band, band + 1, 63, 64, 65, 127, 128, 129, 191, 193}):
        m = rng.integers(1, 1 << 32, n + 1, dtype=np.uint64).astype(np.uint32)
        pos = np.cumsum(rng.integers(20, 60, n + 1))
        reads += [(m, pos), (m, pos + np.cumsum(rng.integers(-2, 3, n + 1)) + 300)]
    an, ch = same_as_model(ctx, pack(reads), pack(reads), band)
    sizes = set(np.diff(an["anchor_offsets"].astype(np.int64)).tolist())
    assert {band, band + 1, 63, 64, 65, 127, 128, 129, 191, 193} - {0} <= sizes | {n for n in (band, band + 1) if n < 10}


def test_a_grid_of_anchors_takes_three_trips(ctx):
    """Two reads that share a tandem repeat of 70 windows: 4 900 anchors a pair (above the LDS share), the diagonal predecessor 70 back;
    band 130 is three trips of 64 lanes, band 62 cuts the diagonal."""
    rng = np.random.default_rng(11)
    a, b = 5, 9
    for band in (130, 62):
        reads = []
        for shift in (0, 1000):
            m = np.concatenate([rng.integers(100, 1 << 32, 12, dtype=np.uint64), np.tile([a, b], 36)[:71], rng.integers(100, 1 << 32, 12, dtype=np.uint64)]).astype(np.uint32)
            reads.append((m, shift + 40 * np.arange(len(m))))
        an, ch = same_as_model(ctx, pack(reads), pack(reads), band)
        assert int(np.diff(an["anchor_offsets"].astype(np.int64)).max()) == 70 * 70
    free = mm.chains(an, None)
    assert (free["chains"]["score"] != ch["chains"]["score"]).any()         # (band 62: the band cut mattered)


def test_a_pair_too_long_to_chain(ctx):
    """460 windows of one pair in each of two reads: 211 600 anchors a pair, above 2^24 / 80 -- flagged, not chained."""
    m = np.tile([21, 22], 231)[:461]
    reads = pack([(m, 40 * np.arange(461)), (m, 7 + 40 * np.arange(461))])
    rows, info, an, ch, chinfo = device(ctx, reads, reads, 62)
    assert list(np.diff(an["anchor_offsets"].astype(np.int64))) == [211600, 211600] and 211600 >= mm.CHAIN_TOO_LONG_FROM
    assert list(ch["chains"]["flags"]) == [mm.CHAIN_TOO_LONG] * 2 and list(ch["chains"]["ref_read"]) == [1, 0]
    for f in ch["chains"].dtype.names[2:]:
        assert not ch["chains"][f].any(), f
    assert list(ch["match_offsets"]) == [0, 0, 0] and chinfo["n_chains"] == 0 and chinfo["n_matches"] == 0
    ix = mm.build_index(*reads)
    mm.same(an, mm.anchors(ix, *reads, min_anchors=1))


def test_2_to_the_32_anchors_are_refused_after_the_count(ctx):
    from metamdbg_amd import capi
    big = np.tile([31, 32], 32769)[:65537]
    rng = np.random.default_rng(5)
    small = rng.integers(100, 1 << 32, 12, dtype=np.uint64)
    chunk = upload(ctx, pack([(big, 40 * np.arange(65537))]))
    queries = upload(ctx, pack([(small, 40 * np.arange(12)), (big, 40 * np.arange(65537))]))
    ix = ctx.map_index_build(chunk, 100)
    assert ix.info()["longest_run"] == 65536
    with pytest.raises(capi.MdbgError) as e:
        ctx.map_anchors(ix, queries, 0, 1)
    assert e.value.code == -5 and "4294967296 anchors" in str(e.value) and "1 query reads from 0 fit" in str(e.value), str(e.value)
    an = ctx.map_anchors(ix, queries, 0, 1, 0, 1)
    assert an.info()["n_anchors"] == 0
    for h in (an, ix, queries, chunk):
        h.free()


def test_refusals(ctx):
    from metamdbg_amd import capi
    m, off, pos = pack([(np.arange(1, 13), 10 * np.arange(1, 13)), (np.arange(5, 20), 10 * np.arange(1, 16))])

    def refused(code, f, *args, **kw):
        with pytest.raises(capi.MdbgError) as e:
            f(*args, **kw)
        assert e.value.code == code, str(e.value)
        return str(e.value)

    bare = ctx.minimizers_from_host(m, off)
    good = ctx.minimizers_with_positions(m, off, pos)
    ix = ctx.map_index_build(good)
    assert "no positions" in refused(-1, ctx.map_index_build, bare)
    assert "no positions" in refused(-1, ctx.map_anchors, ix, bare)
    high = pos.copy(); high[11] = 1 << 31
    assert "read 0, minimizer 11" in refused(-1, bare.attach_positions, high)
    flat = pos.copy(); flat[14] = flat[13]
    assert "read 1, minimizer 2" in refused(-1, bare.attach_positions, flat)
    down = pos.copy(); down[5] = down[4] - 1
    assert "read 0, minimizer 5" in refused(-1, bare.attach_positions, down)
    refused(-1, ctx.map_index_build, bare)                        # a refused attach leaves the set without positions
    refused(-1, ctx.map_index_build, None)
    refused(-1, ctx.map_anchors, None, good)
    refused(-1, ctx.map_anchors, ix, None)
    refused(-1, ctx.map_chains, None)
    assert "outside" in refused(-1, ctx.map_anchors, ix, good, 0, 1, 1, 3)
    assert "outside" in refused(-1, ctx.map_anchors, ix, good, 0, 1, 2, 1)
    refused(-1, ctx.map_anchors, ix, good, 0xFFFFFFFF)             # the queries' global numbers leave 32 bits
    refused(-1, ctx.map_index_build, good, 0xFFFFFFFF)
    an = ctx.map_anchors(ix, good, 0, 1)
    refused(-1, ctx.map_chains, an, 0)
    assert capi.lib().mdbg_map_index_info(None, None) == -1 and capi.lib().mdbg_anchors_info(None, None) == -1 and capi.lib().mdbg_chains_info(None, None) == -1
    bare.attach_positions(pos)                                     # ... and a good attach makes it usable
    ctx.map_index_build(bare).free()
    for h in (an, ix, good, bare):
        h.free()


def test_empty_inputs(ctx):
    none = pack([])
    rng = np.random.default_rng(2)
    some = pack([(rng.integers(1, 1 << 31, 14), 30 * np.arange(14)), (np.zeros(0), np.zeros(0)), (rng.integers(1, 1 << 31, 1), [5]), (rng.integers(1, 1 << 31, 11), 30 * np.arange(11))])
    other = pack([((1 << 31) + rng.integers(1, 1 << 31, 20), 30 * np.arange(20))])
    for chunk, queries in ((none, none), (none, some), (some, none), (some, other), (other, some), (some, some)):
        an, ch = same_as_model(ctx, chunk, queries, 62)
        assert len(an["ref_read"]) == 0 and len(ch["matches"]) == 0 and len(an["pair_offsets"]) == len(queries[1])
    same_as_model(ctx, some, some, 62, query_begin=1, query_end=1)


def test_two_contexts(ctx):
    from metamdbg_amd import capi
    d = mm.load_fixture("band100")
    reads = (d["minimizers"], d["read_offsets"], d["positions"])
    other = capi.Context(0)
    try:
        m1, m2 = upload(ctx, reads), upload(other, reads)
        ix1, ix2 = ctx.map_index_build(m1), other.map_index_build(m2)
        an2 = other.map_anchors(ix2, m2, 0, 3, band=100)
        an1 = ctx.map_anchors(ix1, m1, 0, 3, band=100)
        ch1, ch2 = ctx.map_chains(an1, 100), other.map_chains(an2, 100)
        want_a, want_c = mm.fixture_anchors(d, 3), mm.fixture_chains(d, 3)
        for an, ch in ((an1, ch1), (an2, ch2)):
            mm.same(an.to_host(), want_a)
            mm.same(ch.to_host(), want_c)
        p = an1.device_ptrs()
        assert all(p.values()) and all(ch2.device_ptrs().values())
        for h in (ch2, an2, ix2, m2):
            h.free()
    finally:
        other.close()
    mm.same(ch1.to_host(), want_c)                                # the first context's objects outlive the second context


def test_timers_and_kernel_attributes(ctx):
    d = mm.load_fixture("band5")
    reads = (d["minimizers"], d["read_offsets"], d["positions"])
    ctx.timing(True)
    ctx.timing_reset()
    try:
        device(ctx, reads, reads, 5)
        ctx.synchronize()
        counts = {name: ctx.timing_get(name)[1] for name in ("map_index", "map_count", "map_fill", "map_group", "map_chains", "map_matches", "radix_sort")}
    finally:
        ctx.timing(False)
    assert counts == dict(map_index=1, map_count=1, map_fill=1, map_group=3, map_chains=1, map_matches=1, radix_sort=2), counts
    names = [n for n in ctx.step_kernel_names() if n.startswith("map_")]
    assert len(names) == 15
    for name in names:
        a = ctx.kernel_attributes(name)
        assert a["scratch"] == 0 and a["role"] == 2 and a["static_lds"] == (32768 if name == "map_chain" else 0), (name, a)
