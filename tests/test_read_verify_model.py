"""tests/verify_model.py -- the numpy restatement of mdbg_map_verify's rules (the anchors of a pair in (i, j) order, the chain, its summary,
the identity's table, kept or not) -- against what the REFERENCE's own MinimizerChainer::computeChainingAlignment and the four tests of
filterAlignments computed for tests/golden/read_verify (verify_ref.cpp; make_fixture.py): field for field, verdict for verdict, the kept lists
equal.  The conditions the generator asserted on the fixture are asserted again here, against the counts manifest.json records."""
from __future__ import annotations

import numpy as np
import pytest

from tests import verify_model as vm

CONFIGS = vm.fixture_manifest()["configs"]


@pytest.fixture(scope="module", params=CONFIGS, ids=[c["name"] for c in CONFIGS])
def case(request):
    cfg = request.param
    d = vm.load_fixture(cfg["name"])
    return dict(cfg=cfg, d=d, ref=vm.fixture_verification(d), stats={})


def test_model_equals_the_reference(case):
    d, cfg = case["d"], case["cfg"]
    got = vm.verify(d["sel_offsets"], d["sel_neighbour"], vm.fixture_reads(d), stats=case["stats"], **vm.fixture_params(cfg))
    vm.same(got, case["ref"])
    assert vm.info(got) == dict(n_targets=cfg["n_targets"], n_rows=cfg["rows"], n_chains=cfg["chains"], n_kept=cfg["kept"])
    assert case["stats"].get("pred_ties", 0) > 0 and case["stats"].get("end_ties", 0) > 0


def test_identity_is_the_references_float(case):
    d, cfg = case["d"], case["cfg"]
    rows = case["ref"]["rows"]
    chain = np.flatnonzero(d["row_chain"])
    mine = np.array([vm.identity(int(rows["n_matches"][s]), int(rows["n_seeds"][s]), cfg["minimizer_size"]) for s in chain], np.float32)
    assert np.array_equal(mine.view(np.uint32), d["row_identity"][chain].view(np.uint32))
    table = vm.min_matches(int(rows["n_seeds"].max()), cfg["min_identity"], cfg["minimizer_size"])
    assert np.array_equal(rows["n_matches"][chain] >= table[rows["n_seeds"][chain]], d["row_identity"][chain] >= np.float32(cfg["min_identity"]))
    assert np.all(np.diff(table.astype(np.int64)) >= 0)


def test_fixture_meets_its_conditions(case):
    d, cfg = case["d"], case["cfg"]
    rows = case["ref"]["rows"]
    chain = d["row_chain"] != 0
    over_s, over_e = rows["overhang_start"] > cfg["max_overhang"], rows["overhang_end"] > cfg["max_overhang"]
    short, low = rows["align_length"] < cfg["min_overlap_length"], d["row_identity"] < np.float32(cfg["min_identity"])
    fails = over_s.astype(int) + over_e + short + low
    alone = lambda f: int((chain & f & (fails == 1)).sum())
    kept = d["row_kept"] != 0
    assert np.array_equal(kept, chain & (fails == 0))
    table = vm.min_matches(int(rows["n_seeds"].max()), cfg["min_identity"], cfg["minimizer_size"])
    m = rows["n_matches"].astype(np.int64)
    got = dict(rejected_by_start_overhang_alone=alone(over_s), rejected_by_end_overhang_alone=alone(over_e), rejected_by_length_alone=alone(short),
               rejected_by_identity_alone=alone(low), kept=int(kept.sum()), kept_reversed=int((kept & (rows["query_reversed"] != 0)).sum()),
               rows_3_anchors_up_without_chain=int(((rows["n_anchors"] >= 3) & ~chain).sum()), rows_below_3_anchors=int((rows["n_anchors"] < 3).sum()),
               rows_at_min_matches=int((chain & (m == table[rows["n_seeds"]])).sum()), rows_one_below_min_matches=int((chain & (m + 1 == table[rows["n_seeds"]])).sum()))
    off, so = d["read_offsets"].astype(np.int64), d["sel_offsets"].astype(np.int64)
    target = np.repeat(np.arange(len(so) - 1), np.diff(so))
    multi = 0                                          # rows in which one target minimizer meets several neighbour indexes
    for t, q in zip(target, d["sel_neighbour"]):
        vals, counts = np.unique(d["minimizers"][off[q]:off[q + 1]], return_counts=True)
        multi += bool(np.isin(d["minimizers"][off[t]:off[t + 1]], vals[counts > 1]).any())
    got["rows_with_a_minimizer_meeting_several"] = multi
    assert got == {k: cfg[k] for k in got}
    for k in ("rejected_by_start_overhang_alone", "rejected_by_end_overhang_alone", "rejected_by_length_alone", "rejected_by_identity_alone"):
        assert got[k] >= 20, k
    assert got["kept"] >= 50 and got["kept_reversed"] >= 15
    assert got["rows_3_anchors_up_without_chain"] >= 10 and got["rows_below_3_anchors"] >= 10 and got["rows_with_a_minimizer_meeting_several"] >= 10
    assert got["rows_at_min_matches"] >= 5 and got["rows_one_below_min_matches"] >= 5
    lens = np.diff(d["read_offsets"].astype(np.int64))
    assert lens.min() <= 2 and lens.max() >= 500 and 200 <= len(lens) <= 350


def test_band_cut_changes_chains_between_band_5_and_62():
    """On the band-62 file's reads the model at band 5 leaves other rows: the band is exercised (the generator held the reference to the same)."""
    cfg = next(c for c in CONFIGS if c["band"] == 62)
    assert cfg["rows_changed_between_band_5_and_62"] >= 5
    d = vm.load_fixture(cfg["name"])
    narrow = vm.verify(d["sel_offsets"], d["sel_neighbour"], vm.fixture_reads(d), **dict(vm.fixture_params(cfg), band=5))
    wide = vm.fixture_verification(d)
    differ = np.zeros(len(wide["rows"]), bool)
    for f in ("flags",) + vm.SUMMARY_FIELDS:
        differ |= narrow["rows"][f] != wide["rows"][f]
    assert int(differ.sum()) >= 5


def test_out_of_range_reads_are_absent():
    cfg = CONFIGS[0]
    d = vm.load_fixture(cfg["name"])
    reads = vm.fixture_reads(d)
    n = len(d["read_offsets"]) - 1
    cutat = n // 2
    part = dict(offsets=d["read_offsets"][:cutat + 1], minimizers=reads["minimizers"], positions=reads["positions"], directions=reads["directions"], lengths=reads["lengths"][:cutat])
    got = vm.verify(d["sel_offsets"], d["sel_neighbour"], part, **vm.fixture_params(cfg))
    absent = (got["rows"]["flags"] & vm.VERIFY_ABSENT) != 0
    target = np.repeat(np.arange(n), np.diff(d["sel_offsets"].astype(np.int64)))
    assert np.array_equal(absent, (target >= cutat) | (d["sel_neighbour"] >= cutat))
    whole = vm.fixture_verification(d)["rows"]
    assert np.array_equal(got["rows"][~absent], whole[~absent]) and not got["rows"][absent]["n_matches"].any()
