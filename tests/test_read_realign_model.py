"""tests/realign_model.py -- the numpy restatement of mdbg_map_realign's rules (the density rule, the oriented view of a thinned neighbour, the
anchors, the chain, the alignment list, normalizeAlignment, the entry kinds, the backbone) -- against what the REFERENCE's own
Utils::getLowDensityMinimizerRead, Utils::isReadTooShort, MinimizerRead::toReverseComplement and MinimizerChainer::computeChainingAlignment
computed for tests/golden/read_realign (realign_ref.cpp; make_fixture.py): array for array.  The conditions the generator asserted on the
fixture are asserted again here, against the counts manifest.json records."""
from __future__ import annotations

import os

import numpy as np
import pytest

from tests import realign_model as rm
from tests import verify_model as vm

CONFIGS = rm.fixture_manifest()["configs"]


@pytest.fixture(scope="module", params=CONFIGS, ids=[c["name"] for c in CONFIGS])
def case(request):
    cfg = request.param
    d = rm.load_fixture(cfg["name"])
    stats = {}
    got = rm.realign(d["kept_offsets"], d["kept_neighbour"], d["kept_reversed"], vm.fixture_reads(d), d["qualities"], stats=stats, **rm.fixture_params(cfg))
    return dict(cfg=cfg, d=d, ref=rm.fixture_realignment(d), got=got, stats=stats)


def test_model_equals_the_reference(case):
    rm.same_as_fixture(case["got"], case["ref"])
    cfg = case["cfg"]
    assert rm.info(case["got"]) == dict(n_targets=cfg["n_targets"], n_rows=cfg["kept_rows"], n_chains=cfg["chains"], n_entries=cfg["n_entries"])
    assert case["stats"]["moves"] > 0 and case["stats"]["erased"] > 0          # normalisation moved indexes and erased entries


def test_thinning_is_the_references(case):
    d, cfg = case["d"], case["cfg"]
    keep = rm.thin_keep(d["minimizers"], cfg["density"])
    assert np.array_equal(np.flatnonzero(keep), d["thin_index"]) and int(keep.sum()) == cfg["n_thinned"]


def test_every_file_is_small_and_the_reads_are_read_verifys(case):
    cfg = case["cfg"]
    assert os.path.getsize(os.path.join(rm.FIXTURE_DIR, cfg["name"] + ".npz")) <= 128918
    assert cfg["reads_from"] == "band62" and cfg["seed"] == next(c["seed"] for c in vm.fixture_manifest()["configs"] if c["name"] == "band62")


def test_fixture_meets_its_conditions(case):
    d, cfg, ref = case["d"], case["cfg"], case["ref"]
    rows = ref["rows"]
    state = d["row_state"]
    chain = state == rm.REALIGN_CHAIN
    eo = ref["entry_offsets"].astype(np.int64)
    matches_after = np.array([int((ref["kind"][eo[s]:eo[s + 1]] == rm.MATCH).sum()) for s in range(len(state))])
    assert np.array_equal(d["kept_flipped"], (np.arange(1, len(state) + 1) % rm.fixture_manifest()["flip_every"] == 0).astype(np.uint8))
    off, ko = d["read_offsets"].astype(np.int64), d["kept_offsets"].astype(np.int64)
    keep = np.zeros(int(off[-1]), bool)
    keep[d["thin_index"]] = True
    thin = lambda r: d["minimizers"][off[r]:off[r + 1]][keep[off[r]:off[r + 1]]]
    target = np.repeat(np.arange(len(ko) - 1), np.diff(ko))
    multi = 0
    for t, q, st in zip(target, d["kept_neighbour"], state):
        if st != rm.REALIGN_SHORT:
            vals, counts = np.unique(thin(t), return_counts=True)
            multi += bool(np.isin(thin(int(q)), vals[counts > 1]).any())
    got = dict(kept_rows=len(state), flipped_rows=int(d["kept_flipped"].sum()), short_rows=int((state == rm.REALIGN_SHORT).sum()), rows_without_chain=int((state == 0).sum()),
               chains=int(chain.sum()), reversed_chains=int((chain & (rows["chain_reversed"] != 0)).sum()),
               reversed_chains_unflipped=int((chain & (rows["chain_reversed"] != 0) & (d["kept_flipped"] == 0)).sum()),
               rows_where_normalisation_made_a_match=int((chain & (matches_after > rows["n_matches"])).sum()), longest_list=int(rows["n_entries"].max()),
               lists_above_64_entries=int((rows["n_entries"] > 64).sum()), n_entries=int(eo[-1]), rows_with_a_minimizer_meeting_several=multi)
    assert got == {k: cfg[k] for k in got}
    if cfg["density"] == 0.2:
        assert got["short_rows"] >= 50 and got["rows_without_chain"] >= 40 and got["chains"] >= 300 and got["reversed_chains"] >= 50
        assert got["rows_where_normalisation_made_a_match"] >= 10
    if cfg["density"] == 0.5:
        assert got["lists_above_64_entries"] >= 1
    assert got["rows_with_a_minimizer_meeting_several"] >= 10


def test_the_reversed_branch_is_reached_through_wrong_flags_only():
    """With the verify flag obeyed no chain at band 62 comes out reversed: every reversed chain of those files sits on a flipped row."""
    for cfg in CONFIGS:
        if cfg["band"] == 62:
            assert cfg["reversed_chains"] > 0 and cfg["reversed_chains_unflipped"] == 0


def test_unflipped_flags_are_the_verifiers():
    """The kept rows and the flags given are mdbg_map_verify's own on the same reads and selection (read_verify's fixture holds them at band 62)."""
    v = vm.fixture_verification(vm.load_fixture("band62"))
    for cfg in CONFIGS:
        if cfg["band"] == 62:
            d = rm.load_fixture(cfg["name"])
            assert np.array_equal(v["kept_offsets"], d["kept_offsets"]) and np.array_equal(v["kept_neighbour"], d["kept_neighbour"])
            assert np.array_equal(v["kept_reversed"] ^ d["kept_flipped"], d["kept_reversed"])
