"""mdbg_map_select / mdbg_selection_from_host / mdbg_map_select_merge / mdbg_selection_to_alignment_bytes (csrc/select.hip, select_dev.hpp)
on the device.

Against the REFERENCE: tests/golden/read_select holds what ReadMapper.hpp's own processAnchors / addAlignmentScore selected for seeded reads
at 40-fold coverage with coverage 20, 3 and 1 -- the whole set as one chunk, three chunks, and the chunks merged by its mergeAlignmentScore
(select_ref.cpp; tests/test_read_select_model.py holds the numpy model against the same files).  The device runs reads -> index -> anchors
-> chains -> select, per chunk and merged, and every row and list is compared for equality; so are the alignment file's bytes.

Against the model (tests/select_model.py), on chosen candidates through mdbg_selection_from_host + mdbg_map_select_merge: exactly K and
K + 1 candidates on one position, a tie at the cut, scores <= 0, coverage 1 / 20 / 255 / above the number of candidates, list lengths
63 / 64 / 65 / 129, query extents at the LDS / global seam (from mdbg_select_lds_positions), one query of 3 000 candidates, 5 000 queries
of two, empty queries between full ones, an empty selection; the refusals; two contexts on two host threads.

Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import threading

import numpy as np
import pytest

from tests import select_model as sm

pytestmark = pytest.mark.gpu

MANIFEST = sm.fixture_manifest()
CONFIGS = [(c["name"], c["coverage"]) for c in MANIFEST["configs"]]
BAND = MANIFEST["band"]


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def chains_of(ctx, reads, lo, hi):
    """The chains of every read of `reads` (queries 0 ...) against the chunk of reads [lo, hi): (Chains handle, the handles to free)."""
    mins, off, pos = reads
    a, b = int(off[lo]), int(off[hi])
    qm = ctx.minimizers_with_positions(mins, off, pos)
    cm = ctx.minimizers_with_positions(mins[a:b], off[lo:hi + 1] - off[lo], pos[a:b])
    ix = ctx.map_index_build(cm, lo)
    an = ctx.map_anchors(ix, qm, 0, 3, band=BAND)
    return ctx.map_chains(an, BAND), (an, ix, cm, qm)


def free(*handles):
    for h in handles:
        h.free()


def info_of(sel: dict, n_candidates: int) -> dict:
    return dict(n_queries=len(sel["sel_offsets"]) - 1, n_selected=len(sel["rows"]), n_matches=len(sel["matches"]), n_candidates=n_candidates)


# ---- the reference's fixture ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=CONFIGS, ids=[c[0] for c in CONFIGS])
def case(request, ctx):
    """Computed once per configuration and shared: the whole set's selection, the three chunks', their merge, the alignment bytes."""
    name, coverage = request.param
    d = sm.load_fixture(name)
    reads = (d["minimizers"], d["read_offsets"], d["positions"])
    n = len(d["read_offsets"]) - 1
    ch, rest = chains_of(ctx, reads, 0, n)
    chains = ch.to_host()
    sel = ctx.map_select(ch, coverage)
    whole, whole_info = sel.to_host(), sel.info()
    b = ctx.selection_to_alignment_bytes(sel, 500)
    file_bytes = b.download(0, b.n)
    free(b, sel, ch, *rest)
    bounds = d["chunk_bounds"].tolist()
    parts, part_handles = [], []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        ch, rest = chains_of(ctx, reads, lo, hi)
        part_handles.append(ctx.map_select(ch, coverage))
        parts.append(dict(sel=part_handles[-1].to_host(), chains=ch.to_host()))
        free(ch, *rest)
    m = ctx.map_select_merge(part_handles, coverage)
    merged, merged_info = m.to_host(), m.info()
    free(m, *part_handles)
    return dict(name=name, coverage=coverage, d=d, c=sm.fixture_candidates(d), chains=chains, whole=whole, whole_info=whole_info, file_bytes=file_bytes, parts=parts,
                merged=merged, merged_info=merged_info)


def test_select_against_the_reference(case):
    d, c, got = case["d"], case["c"], case["whole"]
    assert np.array_equal(got["sel_offsets"], d["whole_offsets"]) and np.array_equal(got["rows"]["ref_read"], d["whole_ref_read"])
    want = sm.compact(c, sm.fixture_marks(d, c, "whole"))                 # the reference's rows, scores and lists; pair = the candidate's number
    dev_c = sm.from_chains(case["chains"])                               # ... which the device numbers by its row of the chains
    assert np.array_equal(dev_c["ref_read"], c["ref_read"]) and np.array_equal(dev_c["cand_offsets"], c["cand_offsets"])
    want["rows"]["pair"] = dev_c["pair"][want["rows"]["pair"].astype(np.int64)]
    sm.same(got, want)
    assert case["whole_info"] == info_of(want, len(c["ref_read"]))
    assert 0 < len(want["rows"]) < len(c["ref_read"]) and (want["rows"]["score"] <= 0).any()


def test_chunks_and_merge_against_the_reference(case):
    d, c = case["d"], case["c"]
    for i, p in enumerate(case["parts"]):
        assert np.array_equal(p["sel"]["sel_offsets"], d[f"chunk{i}_offsets"]) and np.array_equal(p["sel"]["rows"]["ref_read"], d[f"chunk{i}_ref_read"]), i
        sm.same(p["sel"], sm.select(sm.from_chains(p["chains"]), case["coverage"]))
    got = case["merged"]
    assert np.array_equal(got["sel_offsets"], d["merged_offsets"]) and np.array_equal(got["rows"]["ref_read"], d["merged_ref_read"])
    want = sm.fixture_merged(d, c)
    for key in ("sel_offsets", "match_offsets", "matches"):
        assert np.array_equal(got[key], want[key]), key
    for f in ("ref_read", "score", "n_matches", "part"):
        assert np.array_equal(got["rows"][f], want["rows"][f]), f
    sm.same(got, sm.merge([p["sel"] for p in case["parts"]], case["coverage"]))          # (pair: the row of the part's own chains, carried through)
    assert case["merged_info"] == info_of(got, sum(len(p["sel"]["rows"]) for p in case["parts"]))
    dropped = sum(len(p["sel"]["rows"]) for p in case["parts"]) - len(got["rows"])
    assert dropped == next(e for e in MANIFEST["configs"] if e["name"] == case["name"])["selected_in_chunk_dropped_by_merge"] >= 5
    # merge == whole
    for f in ("ref_read", "score", "n_matches"):
        assert np.array_equal(got["rows"][f], case["whole"]["rows"][f]), f
    assert np.array_equal(got["matches"], case["whole"]["matches"])


def test_alignment_bytes_against_the_fixture(case):
    d, c = case["d"], case["c"]
    want = sm.alignment_bytes(sm.compact(c, sm.fixture_marks(d, c, "whole")), 500)
    assert case["file_bytes"] == want and len(want) == 8 * int((np.diff(d["whole_offsets"].astype(np.int64)) > 0).sum()) + 4 * len(d["whole_ref_read"])


# ---- chosen candidates through mdbg_selection_from_host + mdbg_map_select_merge -------------------------------------------------------------
def pack(queries: list) -> dict:
    """[[(ref_read, list), ...] per query] -> the candidates"""
    co, ref, mo, matches = [0], [], [0], []
    for q in queries:
        for r, lst in q:
            ref.append(r)
            matches.append(np.asarray(lst, np.uint32))
            mo.append(mo[-1] + len(lst))
        co.append(len(ref))
    return sm.from_lists(co, ref, mo, np.concatenate(matches) if matches else np.zeros(0, np.uint32))


def upload(ctx, c: dict):
    return ctx.selection_from_host(c["cand_offsets"], c["ref_read"], c["match_offsets"], c["matches"])


def device_select(ctx, c: dict, coverage: int) -> dict:
    """The candidates stored (from_host: every row kept, the scores computed by the library) and selected by a one-part merge."""
    part = upload(ctx, c)
    stored = part.to_host()
    sm.same(stored, sm.compact(c, np.ones(len(c["ref_read"]), bool)))
    assert part.info() == info_of(stored, len(c["ref_read"]))
    m = ctx.map_select_merge([part], coverage)
    got = m.to_host()
    assert m.info() == info_of(got, len(c["ref_read"]))
    b = ctx.selection_to_alignment_bytes(m, 7)
    assert b.download(0, b.n) == sm.alignment_bytes(got, 7)
    free(b, m, part)
    return got


def same_as_model(ctx, queries: list, coverage: int) -> dict:
    c = pack(queries)
    got = device_select(ctx, c, coverage)
    sm.same(got, sm.select(c, coverage))
    return got


@pytest.mark.parametrize("coverage", [1, 3, 20, 255])
def test_k_and_k_plus_1_on_one_position_and_a_tie_at_the_cut(ctx, coverage):
    k = coverage
    run = lambda first, n: list(range(first, first + n))
    exactly_k = [(10 + i, [5, 6 + i]) for i in range(k)]                                  # K on position 5: all stay
    k_plus_1 = [(10 + i, run(5, 3 + (i == 0))) for i in range(k + 1)]                     # K + 1 on 5, 6, 7; read 10 scores 4, the rest tie at 3: the largest read leaves
    tie = [(1, run(40, 4))] + [(3 + 2 * i, run(40, 4)) for i in range(k)] + [(1001, run(40, 4))]      # K + 2 with one score: the two largest reads leave
    low = [(7 + i, [2, 9 + 4 * i, 30 + 9 * i]) for i in range(k + 3)]                     # scores 6 - span, all <= 0 and falling: the last three leave position 2 ...
    got = same_as_model(ctx, [exactly_k, k_plus_1, [], tie, low], coverage)
    so = got["sel_offsets"].astype(np.int64)
    reads = lambda q: got["rows"]["ref_read"][so[q]:so[q + 1]].tolist()
    assert reads(0) == [10 + i for i in range(k)]
    assert reads(1) == [10 + i for i in range(k)] and got["rows"]["score"][so[1]] == 4
    assert reads(2) == [] and reads(3) == sorted([1] + [3 + 2 * i for i in range(k)])[:k]
    assert len(reads(4)) == k + 3 and (got["rows"]["score"][so[4]:so[5]] <= 0).all()     # ... but each keeps a position of its own


def test_coverage_above_the_number_of_candidates(ctx):
    rng = np.random.default_rng(1)
    q = [(int(r), np.sort(rng.choice(50, 9, replace=False))) for r in np.sort(rng.choice(1000, 30, replace=False))]
    for coverage in (31, 255):
        assert len(same_as_model(ctx, [q], coverage)["rows"]) == 30
    assert len(same_as_model(ctx, [q], 1)["rows"]) < 30


@pytest.mark.parametrize("coverage", [1, 20])
def test_list_lengths_at_the_wave(ctx, coverage):
    """Lists of 63, 64, 65 and 129 elements (one, one, two and three trips of 64 lanes), each the only one to cover its LAST position."""
    rng = np.random.default_rng(coverage)
    q, r = [], 0
    for n in (63, 64, 65, 129, 1, 128):
        for j in range(coverage + 2):          # coverage + 2 lists of one score over the same stretch ...
            q.append((r, list(range(100, 100 + n))))
            r += 1 + int(rng.integers(0, 3))
        q.append((r, list(range(101, 101 + n))))       # ... and one that is taken by its last element alone (a dropped partial trip would lose it)
        r += 1
        q.sort()
        got = same_as_model(ctx, [q], coverage)
        assert q[-1][0] in got["rows"]["ref_read"].tolist()
        q = []


def test_query_extents_at_the_lds_seam(ctx):
    """Queries whose positions end at SELECT_LDS_POSITIONS - 1, at it and above it: counters in LDS, in LDS, in the pooled global buffer."""
    lds = ctx.select_lds_positions()
    assert lds >= 1024
    rng = np.random.default_rng(lds)
    queries = []
    for extent in (lds - 1, lds, lds + 1, 3 * lds + 5, 40):
        q = []
        for i in range(25):
            n = int(rng.integers(3, 200))
            first = int(rng.integers(0, extent - 400))  if extent > 1000 else 0
            q.append((2 * i, np.sort(first + rng.choice(min(extent, 400), min(n, extent // 2), replace=False))))
        for i in range(25, 29):                # four candidates that end on the query's last position: coverage 3 drops the lowest
            q.append((2 * i, list(range(extent - 3 - i, extent))))
        queries.append(q)
    for coverage in (3, 20):
        got = same_as_model(ctx, queries, coverage)
        so = got["sel_offsets"].astype(np.int64)
        for qi in range(4):
            assert (50 in got["rows"]["ref_read"][so[qi]:so[qi + 1]].tolist()) == (coverage == 20)       # the shortest of the four: rank 4 on the last position


def test_one_query_of_3000_candidates(ctx):
    rng = np.random.default_rng(3000)
    q = []
    for r in range(3000):
        n = int(rng.integers(1, 70))
        first = int(rng.integers(0, 300))
        q.append((3 * r + 1, np.sort(first + rng.choice(n + int(rng.integers(0, 20)), n, replace=False))))
    for coverage in (1, 20, 255):
        got = same_as_model(ctx, [[], q, []], coverage)
        assert 0 < len(got["rows"]) < 3000


def test_5000_queries_of_two_candidates(ctx):
    """More queries than resident waves: every wave draws many, empty ones between full ones."""
    rng = np.random.default_rng(5000)
    queries = []
    for i in range(5000):
        if i % 7 == 3:
            queries.append([])
            continue
        a = int(rng.integers(0, 60))
        queries.append([(i, list(range(a, a + 5))), (i + 9, list(range(a + 2, a + 5 + int(rng.integers(0, 4)))))])
    got = same_as_model(ctx, queries, 1)
    assert 4285 < len(got["rows"]) < 2 * 4286
    assert len(same_as_model(ctx, queries, 2)["rows"]) == 2 * 4286


def test_merge_is_the_whole_on_a_seeded_set(ctx):
    from tests.test_read_select_model import seeded_candidates
    c = seeded_candidates(11, n_queries=60)
    for coverage, bounds in ((3, [0, 30, 60, 90]), (20, [0, 45, 90])):
        chunks = sm.split_by_read(c, bounds)
        stored = [upload(ctx, ch) for ch in chunks]
        parts = [ctx.map_select_merge([s], coverage) for s in stored]
        m = ctx.map_select_merge(parts, coverage)
        got = m.to_host()
        sm.same(got, sm.merge([p.to_host() for p in parts], coverage))
        whole = device_select(ctx, c, coverage)
        for key in ("sel_offsets", "match_offsets", "matches"):
            assert np.array_equal(got[key], whole[key]), key
        for f in ("ref_read", "score", "n_matches"):
            assert np.array_equal(got["rows"][f], whole["rows"][f]), f
        assert set(got["rows"]["part"].tolist()) == set(range(len(bounds) - 1))
        free(m, *parts, *stored)


def test_empty_inputs(ctx):
    none = same_as_model(ctx, [], 20)
    assert list(none["sel_offsets"]) == [0] and list(none["match_offsets"]) == [0]
    blank = same_as_model(ctx, [[], [], []], 20)
    assert list(blank["sel_offsets"]) == [0, 0, 0, 0] and len(blank["rows"]) == 0
    a, b = upload(ctx, pack([[], [(4, [1, 2])]])), upload(ctx, pack([[], []]))
    m = ctx.map_select_merge([b, a, b], 5)
    got = m.to_host()
    assert list(got["sel_offsets"]) == [0, 0, 1] and list(got["rows"]["part"]) == [1] and list(got["matches"]) == [1, 2]
    e = ctx.map_select_merge([b, b], 5)
    assert e.info() == dict(n_queries=2, n_selected=0, n_matches=0, n_candidates=0)
    by = ctx.selection_to_alignment_bytes(e)
    assert by.n == 0
    # chains without a single chain: an empty selection
    mins = np.arange(1, 25, dtype=np.uint32)
    m0 = ctx.minimizers_with_positions(mins, np.array([0, 12, 24], np.uint64), np.tile(30 * np.arange(12), 2).astype(np.uint32))
    ix = ctx.map_index_build(m0)
    an = ctx.map_anchors(ix, m0, 0, 3)
    ch = ctx.map_chains(an, 62)
    s = ctx.map_select(ch, 20)
    assert s.info() == dict(n_queries=2, n_selected=0, n_matches=0, n_candidates=0) and list(s.to_host()["sel_offsets"]) == [0, 0, 0]
    assert all(s.device_ptrs().values())
    free(s, ch, an, ix, m0, by, e, m, a, b)


def test_refusals(ctx):
    from metamdbg_amd import capi

    def refused(f, *args):
        with pytest.raises(capi.MdbgError) as e:
            f(*args)
        assert e.value.code == -1, str(e.value)
        return str(e.value)

    good = pack([[(1, [1, 2, 3])], [(2, [4, 9]), (5, [0, 7])]])
    a = upload(ctx, good)
    for coverage in (0, 256):
        assert "coverage" in refused(ctx.map_select_merge, [a], coverage)
    three = upload(ctx, pack([[], [], []]))
    assert "queries" in refused(ctx.map_select_merge, [a, three], 20)
    # the reads of query 1 do not ascend across the parts: part 1 starts at read 5 again
    again = upload(ctx, pack([[(9, [1])], [(5, [3, 4])]]))
    assert "query 1" in refused(ctx.map_select_merge, [a, again], 20)
    back = upload(ctx, pack([[(0, [1])], [(6, [3, 4])]]))
    assert "query 0" in refused(ctx.map_select_merge, [a, back], 20)
    ok = ctx.map_select_merge([a, upload(ctx, pack([[(2, [8])], [(6, [3, 4])]]))], 20)
    assert list(ok.to_host()["rows"]["ref_read"]) == [1, 2, 2, 5, 6]
    refused(ctx.map_select_merge, [], 20)
    refused(ctx.map_select_merge, [a, None], 20)
    refused(ctx.map_select, None, 20)
    so, rr, mo = [0, 1, 3], [1, 2, 5], [0, 3, 5, 7]
    assert "query 1" in refused(ctx.selection_from_host, so, rr, mo, [1, 2, 3, 4, 4, 0, 7])          # a list that does not ascend strictly
    assert "query 1" in refused(ctx.selection_from_host, so, rr, mo, [1, 2, 3, 4, 9, 7, 0])
    assert "query 0" in refused(ctx.selection_from_host, so, rr, [0, 0, 5, 7], [1, 2, 3, 4, 9, 0, 7])       # an empty list
    assert "query 1" in refused(ctx.selection_from_host, so, [1, 5, 5], mo, [1, 2, 3, 4, 9, 0, 7])          # reads that do not ascend strictly
    assert "query 1" in refused(ctx.selection_from_host, [0, 2, 1], rr, mo, [1, 2, 3, 4, 9, 0, 7])          # offsets that do not ascend
    assert "query 1" in refused(ctx.selection_from_host, so, rr, [0, 3, 2, 7], [1, 2, 3, 4, 9, 0, 7])
    assert capi.lib().mdbg_selection_info(None, None) == -1 and capi.lib().mdbg_selection_device_ptrs(None, None) == -1
    # coverage on mdbg_map_select itself
    mins = np.arange(1, 25, dtype=np.uint32)
    m0 = ctx.minimizers_with_positions(mins, np.array([0, 12, 24], np.uint64), np.tile(30 * np.arange(12), 2).astype(np.uint32))
    ix = ctx.map_index_build(m0)
    an = ctx.map_anchors(ix, m0, 0, 3)
    ch = ctx.map_chains(an, 62)
    for coverage in (0, 256):
        assert "coverage" in refused(ctx.map_select, ch, coverage)
    refused(ctx.selection_to_alignment_bytes, None)
    refused(ctx.selection_to_alignment_bytes, a, 0xFFFFFFFF)
    free(ch, an, ix, m0, ok, back, again, three, a)


def test_two_contexts_on_two_threads():
    """Each thread its own context: the fixture's whole-set selection and a chosen set, at the same time."""
    from metamdbg_amd import capi
    d = sm.load_fixture("coverage3")
    c = sm.fixture_candidates(d)
    want = sm.fixture_marks(d, c, "whole")
    reads = (d["minimizers"], d["read_offsets"], d["positions"])
    errors, results = [], [None, None]

    def work(slot):
        try:
            cx = capi.Context(0)
            try:
                for _ in range(3):
                    ch, rest = chains_of(cx, reads, 0, len(d["read_offsets"]) - 1)
                    sel = cx.map_select(ch, 3)
                    results[slot] = sel.to_host()
                    stored = upload(cx, c)
                    m = cx.map_select_merge([stored], 3)
                    assert np.array_equal(m.to_host()["rows"]["ref_read"], results[slot]["rows"]["ref_read"])
                    free(m, stored, sel, ch, *rest)
            finally:
                cx.close()
        except Exception as e:       # noqa: BLE001 -- handed to the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for got in results:
        assert np.array_equal(got["sel_offsets"], d["whole_offsets"]) and np.array_equal(got["rows"]["ref_read"], d["whole_ref_read"])
        assert np.array_equal(got["rows"]["ref_read"], c["ref_read"][want])


def test_timers_and_kernel_attributes(ctx):
    c = pack([[(i, [1, 2, 3 + i]) for i in range(30)]])
    part = upload(ctx, c)
    ctx.timing(True)
    ctx.timing_reset()
    try:
        m = ctx.map_select_merge([part], 3)
        ctx.synchronize()
        counts = {name: ctx.timing_get(name)[1] for name in ("map_select", "radix_sort")}
    finally:
        ctx.timing(False)
    assert counts == dict(map_select=4, radix_sort=1), counts
    free(m, part)
    names = [n for n in ctx.step_kernel_names() if n.startswith("select")]
    assert len(names) == 12
    for name in names:
        a = ctx.kernel_attributes(name)
        assert a["scratch"] == 0 and a["role"] == 2 and a["static_lds"] == (4 * ctx.select_lds_positions() if name == "select" else 0), (name, a)
