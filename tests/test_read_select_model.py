"""tests/select_model.py -- the numpy restatement of the per-position selection -- against what the REFERENCE selected
(tests/golden/read_select: ReadMapper.hpp's own processAnchors / addAlignmentScore and mergeAlignmentScore, run by select_ref.cpp), array
for array: the whole set as one chunk, each of three chunks, the chunks merged.  The closed form (``select``) and the heap procedure
(``heaps``) are both held against it, the fixture's conditions are asserted again, and merge(select(chunk_i)) == select(all) is checked on
the fixture's candidates and on seeded sets."""
from __future__ import annotations

import numpy as np
import pytest

from tests import mapper_model as mm
from tests import select_model as sm

MANIFEST = sm.fixture_manifest()
CONFIGS = [(c["name"], c["coverage"]) for c in MANIFEST["configs"]]
CONDITIONS = ("queries_with_a_position_above_coverage", "positions_tied_at_the_cut", "selected_through_one_position", "took_part_selected_nowhere",
              "pushed_and_evicted_everywhere", "selected_in_chunk_dropped_by_merge", "candidates_scoring_0_or_less")


@pytest.fixture(scope="module", params=CONFIGS, ids=[c[0] for c in CONFIGS])
def case(request):
    name, coverage = request.param
    d = sm.load_fixture(name)
    c = sm.fixture_candidates(d)
    return dict(name=name, coverage=coverage, d=d, c=c, entry=next(e for e in MANIFEST["configs"] if e["name"] == name))


def test_configurations():
    assert sorted(c[1] for c in CONFIGS) == [1, 3, 20] and MANIFEST["band"] == 62 and MANIFEST["chunks"] == 3


def test_one_score_serves_both_entry_points(case):
    """n_matches - n_diff_query of the chain (:1241) is 2 n - (last - first + 1) of its list (:376-382); the lists ascend strictly."""
    c = case["c"]
    assert np.array_equal(sm.list_scores(c["match_offsets"], c["matches"]), c["score"])
    inner = np.ones(len(c["matches"]), bool)
    inner[c["match_offsets"][:-1].astype(np.int64)] = False
    assert (np.diff(c["matches"].astype(np.int64), prepend=0)[inner] > 0).all()


def test_whole_set_against_the_reference(case):
    c, d = case["c"], case["d"]
    want = sm.fixture_marks(d, c, "whole")
    assert np.array_equal(sm.marks(c, case["coverage"]), want)
    assert np.array_equal(sm.heaps(c, case["coverage"]), want)
    sel = sm.select(c, case["coverage"])
    assert np.array_equal(sel["sel_offsets"], d["whole_offsets"]) and np.array_equal(sel["rows"]["ref_read"], d["whole_ref_read"])
    assert len(sel["rows"]) == case["entry"]["n_selected"] < case["entry"]["n_candidates"] == len(c["ref_read"])


def test_chunks_and_merge_against_the_reference(case):
    c, d, k = case["c"], case["d"], case["coverage"]
    chunks = sm.split_by_read(c, d["chunk_bounds"].tolist())
    mine = [sm.select(ch, k) for ch in chunks]
    theirs = sm.fixture_chunks(d, c)
    for a, b in zip(mine, theirs):
        sm.same(a, b)
    merged = sm.merge(theirs, k)
    sm.same(merged, sm.fixture_merged(d, c))
    assert len({int(p) for p in merged["rows"]["part"]}) == 3
    # selecting per chunk and merging is one selection over all chunks' chains
    whole = sm.select(c, k)
    for key in ("sel_offsets", "match_offsets", "matches"):
        assert np.array_equal(merged[key], whole[key]), key
    for f in ("ref_read", "score", "n_matches", "pair"):
        assert np.array_equal(merged["rows"][f], whole["rows"][f]), f
    # a one-part merge at a lower coverage re-selects
    again = sm.merge([whole], 1)
    lower = sm.select(c, 1)
    assert np.array_equal(again["rows"]["pair"], lower["rows"]["pair"]) and np.array_equal(again["sel_offsets"], lower["sel_offsets"])


def test_conditions(case):
    c, d, k = case["c"], case["d"], case["coverage"]
    parts = sm.fixture_chunks(d, c)
    got = sm.conditions(c, k, parts, sm.fixture_marks(d, sm.concat(parts), "merged"))
    assert got == {name: case["entry"][name] for name in CONDITIONS}


def test_candidates_are_the_found_chains():
    """The fixture's candidates are the MDBG_CHAIN_FOUND rows of the mapper model's chains (on a slice of queries: the model is a Python loop)."""
    d = sm.load_fixture("coverage1")
    c = sm.fixture_candidates(d)
    reads = (d["minimizers"], d["read_offsets"], d["positions"])
    ix = mm.build_index(*reads)
    an = mm.anchors(ix, *reads, min_anchors=3, query_begin=20, query_end=32)
    got = sm.from_chains(mm.chains(an, 62))
    co = c["cand_offsets"].astype(np.int64)
    a, b = co[20], co[32]
    assert b - a > 200
    assert np.array_equal(got["cand_offsets"], c["cand_offsets"][20:33] - c["cand_offsets"][20])
    assert np.array_equal(got["ref_read"], c["ref_read"][a:b]) and np.array_equal(got["score"], c["score"][a:b])
    mo = c["match_offsets"].astype(np.int64)
    assert np.array_equal(got["matches"], c["matches"][mo[a]:mo[b]])


def seeded_candidates(seed: int, n_queries: int = 40, n_reads: int = 90, extent: int = 120):
    rng = np.random.default_rng(seed)
    co, ref, mo, matches = [0], [], [0], []
    for q in range(n_queries):
        reads = np.sort(rng.choice(n_reads, int(rng.integers(1, n_reads)) if q % 5 != 4 else 0, replace=False))       # (every fifth query has no candidate)
        for r in reads:
            n = int(rng.integers(1, 40))
            first = int(rng.integers(0, extent - n))
            span = min(extent - first, n + int(rng.integers(0, n + 3)))
            matches.extend(np.sort(first + rng.choice(span, n, replace=False)).tolist())
            mo.append(len(matches))
        ref.extend(reads.tolist())
        co.append(len(ref))
    return sm.from_lists(co, ref, mo, matches)


@pytest.mark.parametrize("seed,coverage,bounds", [(1, 1, [0, 30, 60, 90]), (2, 3, [0, 45, 90]), (3, 20, [0, 10, 20, 80, 90]), (4, 255, [0, 1, 90])])
def test_merge_of_the_chunks_is_the_whole_on_seeded_sets(seed, coverage, bounds):
    c = seeded_candidates(seed)
    whole = sm.select(c, coverage)
    assert np.array_equal(sm.heaps(c, coverage), sm.marks(c, coverage))
    merged = sm.merge([sm.select(ch, coverage) for ch in sm.split_by_read(c, bounds)], coverage)
    for key in ("sel_offsets", "match_offsets", "matches"):
        assert np.array_equal(merged[key], whole[key]), key
    for f in ("ref_read", "score", "n_matches", "pair"):
        assert np.array_equal(merged["rows"][f], whole["rows"][f]), f
    assert (c["score"] <= 0).any() and (coverage == 255 or len(whole["rows"]) < len(c["ref_read"]))


def test_alignment_bytes():
    c = seeded_candidates(7, n_queries=12)
    sel = sm.select(c, 2)
    b = np.frombuffer(sm.alignment_bytes(sel, 1000), "<u4")
    so = sel["sel_offsets"].astype(np.int64)
    at = 0
    for q in range(12):
        n = so[q + 1] - so[q]
        if n == 0:
            continue
        assert b[at] == 1000 + q and b[at + 1] == n and np.array_equal(b[at + 2:at + 2 + n], sel["rows"]["ref_read"][so[q]:so[q + 1]])
        at += 2 + n
    assert at == len(b) and (np.diff(so) == 0).any()
