"""The numpy restatement of the read mapper (tests/mapper_model.py) against what the REFERENCE computed (tests/golden/read_mapper, written
by mapper_ref.cpp from ReadMapper.hpp's own ReadFunctor, sortParallel, createLookupTable and chainAnchors): index, anchors and chains,
array for array, for the three bands -- and the conditions on the fixture's selection, counted again."""
from __future__ import annotations

import numpy as np
import pytest

from tests import mapper_model as mm

CONFIGS = [(c["name"], c["band"]) for c in mm.fixture_manifest()["configs"]]


@pytest.fixture(scope="module", params=CONFIGS, ids=[c[0] for c in CONFIGS])
def case(request):
    name, band = request.param
    d = mm.load_fixture(name)
    ix = mm.build_index(d["minimizers"], d["read_offsets"], d["positions"])
    an = mm.anchors(ix, d["minimizers"], d["read_offsets"], d["positions"], min_anchors=1)
    stats = {}
    ch = mm.chains(an, band, stats)
    return dict(name=name, band=band, d=d, ix=ix, an=an, ch=ch, stats=stats)


def test_three_bands():
    assert sorted(b for _, b in CONFIGS) == [5, 62, 100]


def test_index_is_the_references_per_pair(case):
    d, ix = case["d"], case["ix"]
    # the reference's order inside a pair is whatever its sort left: compared as sorted rows
    ref = np.lexsort((d["index_index"], d["index_read"], d["index_pair"]))
    assert np.array_equal(d["index_pair"], np.sort(d["index_pair"]))
    for mine, theirs in (("pair", "index_pair"), ("read", "index_read"), ("position", "index_position"), ("index", "index_index"), ("reversed", "index_reversed")):
        assert np.array_equal(ix[mine], d[theirs][ref]), mine
    lens = np.diff(d["read_offsets"].astype(np.int64))
    assert len(ix["pair"]) == int(np.maximum(lens - 1, 0).sum())          # reads below 10 minimizers are in the index too


def test_anchors_are_the_references(case):
    mm.same(case["an"], mm.fixture_anchors(case["d"], 1))
    assert np.array_equal(np.diff(case["an"]["pair_offsets"].astype(np.int64)) > 0, case["d"]["query_anchors"] > 0)


def test_min_anchors_3_drops_what_process_anchors_drops(case):
    d = case["d"]
    an3 = mm.anchors(case["ix"], d["minimizers"], d["read_offsets"], d["positions"], min_anchors=3)
    mm.same(an3, mm.fixture_anchors(d, 3))


def test_chains_are_the_references(case):
    mm.same(case["ch"], mm.fixture_chains(case["d"], 1))


def test_conditions_on_the_selection(case):
    d, band, ch = case["d"], case["band"], case["ch"]
    rec = next(c for c in mm.fixture_manifest()["configs"] if c["name"] == case["name"])
    found = d["pair_score"] != 0
    pa = d["pair_anchors"].astype(np.int64)
    assert int((found & (d["chain_query_reversed"] == 1)).sum()) == rec["chains_query_reversed"] >= 50
    assert int((found & (d["chain_query_reversed"] == 0)).sum()) == rec["chains_query_forward"] >= 50
    assert int((pa < 3).sum()) == rec["pairs_below_3"] >= 20
    assert int(((pa >= 3) & ~found).sum()) == rec["pairs_3_up_without_chain"] >= 20
    ao = np.concatenate([[0], np.cumsum(pa)])
    assert sum(1 for p in range(len(pa)) if len(set(d["anchor_reversed"][ao[p]:ao[p + 1]].tolist())) == 2) == rec["pairs_mixing_strands"] >= 10
    assert rec["short_queries_hitting"] >= 5 and rec["reads_hitting_own_windows"] >= 5
    assert int(pa.max()) == rec["longest_pair"] > band + 64
    lens = np.diff(d["read_offsets"].astype(np.int64))
    assert {0, 1, 2, 9} <= set(lens.tolist())
    w = mm.windows(d["minimizers"], d["read_offsets"], d["positions"])
    assert int((w["reversed"] == 1).sum()) > 0 and bool(((w["pair"] >> np.uint64(32)) == (w["pair"] & np.uint64(0xFFFFFFFF))).any())     # windows with a == b
    assert case["stats"]["pred_ties"] == rec["anchors_with_tied_predecessors"] >= 10
    assert case["stats"]["end_ties"] == rec["pairs_with_tied_best"] >= 3
    free = mm.chains(case["an"], None)
    assert int((free["chains"]["score"] != ch["chains"]["score"]).sum()) == rec["pairs_changed_by_the_band"] >= 3
