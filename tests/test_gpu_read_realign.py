"""mdbg_minimizers_attach_qualities / mdbg_map_realign / mdbg_map_realign_pairs (csrc/realign.hip, realign_dev.hpp) on the device.  Everything
is compared for exact equality: the data is integers, there is no tolerance.

Against the REFERENCE: tests/golden/read_realign holds what Utils::getLowDensityMinimizerRead, Utils::isReadTooShort,
MinimizerRead::toReverseComplement and MinimizerChainer::computeChainingAlignment (normalizeAlignment included) computed for the kept rows of
seeded reads at (band 62, density 0.2), (band 5, 0.2) and (band 62, 0.5), every fourth flag flipped (realign_ref.cpp;
tests/test_read_realign_model.py holds the numpy model against the same files).

Against the model (tests/realign_model.py), on inputs the fixture does not have: the kept lists read on the device behind mdbg_map_verify,
a real scan output, and pairs built so that a length is exact -- raw lists of L - 1, L and L + 1 entries for the L of
mdbg_realign_lds_entries with indels planted beside equal values, chains of 63, 64 and 65 links, thinned neighbours of 9, 10 and 11
minimizers, a reversed neighbour of 1 023, 1 024 and 1 025 thinned minimizers that carries one value three times, the cascade
tests/host/test_realign.cpp prints -- targets without a kept row, with an empty thinned form and outside the reads, a set without qualities,
refusals, empty inputs, two contexts on two threads.

Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import threading

import numpy as np
import pytest

from tests import realign_model as rm
from tests import verify_model as vm

pytestmark = pytest.mark.gpu

CONFIGS = rm.fixture_manifest()["configs"]
DENSITY = 0.5          # of the built pairs: half the drawn values stay, so a pair's thinned lengths are chosen value by value


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def upload(ctx, reads: dict, qualities=None):
    m = ctx.minimizers_with_strands(reads["minimizers"], reads["offsets"], reads["positions"], reads["directions"], reads["lengths"])
    if qualities is not None:
        m.attach_qualities(qualities)
    return m


def device_pairs(ctx, kept_offsets, kept_neighbour, kept_reversed, reads: dict, qualities=None, **kw) -> tuple:
    m = upload(ctx, reads, qualities)
    r = ctx.map_realign_pairs(kept_offsets, kept_neighbour, kept_reversed, m, kw.pop("target_first_read", 0), kw.pop("reads_first_read", 0), kw["band"], kw["density"],
                              kw["min_minimizers"])
    out = r.to_host(), r.info()
    r.free(); m.free()
    return out


def pack(reads: list) -> tuple:
    """[(minimizers, positions, directions, length, qualities), ...] -> the model's dict and the qualities"""
    cat = lambda k, t: np.concatenate([np.asarray(r[k], t) for r in reads]) if reads else np.zeros(0, t)
    return dict(offsets=np.concatenate([[0], np.cumsum([len(r[0]) for r in reads])]).astype(np.uint64), minimizers=cat(0, np.uint32), positions=cat(1, np.uint32),
                directions=cat(2, np.uint8), lengths=np.array([r[3] for r in reads], np.uint32)), cat(4, np.uint8)


# ---- the reference's fixture ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=CONFIGS, ids=[c["name"] for c in CONFIGS])
def case(request, ctx):
    cfg = request.param
    d = rm.load_fixture(cfg["name"])
    got, info = device_pairs(ctx, d["kept_offsets"], d["kept_neighbour"], d["kept_reversed"], vm.fixture_reads(d), d["qualities"], **rm.fixture_params(cfg))
    return dict(cfg=cfg, d=d, got=got, info=info)


def test_rows_lists_and_backbone_against_the_reference(case):
    cfg = case["cfg"]
    rm.same_as_fixture(case["got"], rm.fixture_realignment(case["d"]))
    assert case["info"] == dict(n_targets=cfg["n_targets"], n_rows=cfg["kept_rows"], n_chains=cfg["chains"], n_entries=cfg["n_entries"])
    assert cfg["reversed_chains"] >= 50 and cfg["chains"] >= 300


def test_behind_the_verifier_on_the_device(ctx):
    """mdbg_map_verify -> mdbg_map_realign, the kept lists never leaving the device, equals mdbg_map_realign_pairs fed the downloaded lists,
    and the model; the flags are the verifier's own (none flipped)."""
    cfg = CONFIGS[0]
    d = rm.load_fixture(cfg["name"])
    v_cfg = next(c for c in vm.fixture_manifest()["configs"] if c["name"] == cfg["reads_from"])
    dv = vm.load_fixture(v_cfg["name"])
    reads = vm.fixture_reads(d)
    m = upload(ctx, reads, d["qualities"])
    n = len(dv["sel_neighbour"])
    sel = ctx.selection_from_host(dv["sel_offsets"], dv["sel_neighbour"], np.arange(n + 1, dtype=np.uint64), np.zeros(n, np.uint32))
    v = ctx.map_verify(sel, m, **vm.fixture_params(v_cfg))
    kept = v.to_host()
    r = ctx.map_realign(v, m, 0, 0, cfg["band"], cfg["density"], cfg["min_minimizers"])
    on_device = r.to_host()
    r.free()
    r = ctx.map_realign_pairs(kept["kept_offsets"], kept["kept_neighbour"], kept["kept_reversed"], m, 0, 0, cfg["band"], cfg["density"], cfg["min_minimizers"])
    rm.same(on_device, r.to_host())
    for h in (r, v, sel, m):
        h.free()
    assert np.array_equal(kept["kept_neighbour"], d["kept_neighbour"]) and np.array_equal(kept["kept_reversed"] ^ d["kept_flipped"], d["kept_reversed"])
    rm.same(on_device, rm.realign(kept["kept_offsets"], kept["kept_neighbour"], kept["kept_reversed"], reads, d["qualities"], **rm.fixture_params(cfg)))
    chain = (on_device["rows"]["flags"] & rm.REALIGN_CHAIN) != 0
    assert int(chain.sum()) >= 300 and not on_device["rows"]["chain_reversed"][chain].any()
    same_rows = d["kept_flipped"] == 0              # the rows whose flag the fixture left alone are the fixture's
    assert np.array_equal(on_device["rows"][same_rows], rm.fixture_realignment(d)["rows"][same_rows])


# ---- a scan output ---------------------------------------------------------------------------------------------------------------------------
def test_backbone_of_a_scan_output_is_its_thresholded_form(ctx):
    rng = np.random.default_rng(11)
    seqs = [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(n))]) for n in (6000, 40, 9000, 7000)]
    quals = [bytes((33 + rng.integers(5, 40, len(s))).astype(np.uint8)) for s in seqs]
    rd = ctx.reads_from_ascii(seqs, quals)
    m = ctx.scan(rd, K=15, density=0.05, hpc=False, apply_read_filters=False)
    r = ctx.map_realign_pairs(np.array([0, 1, 1, 2, 2], np.uint64), np.array([2, 0], np.uint32), np.array([0, 1], np.uint8), m, 0, 0, 62, 0.01, 10)     # the fresh scan output
    got = r.to_host()
    thin = ctx.apply_density_threshold(m, 0.01)
    t, full = thin.to_host(), m.to_host()
    assert np.array_equal(got["target_offsets"], t["offsets"]) and np.array_equal(got["target_minimizer"], t["minimizers"]) and np.array_equal(got["target_quality"], t["qual"])
    assert 0 < len(t["minimizers"]) < len(full["minimizers"]) and len(set(t["qual"].tolist())) > 1
    reads = dict(offsets=full["offsets"], minimizers=full["minimizers"], positions=full["pos"], directions=full["dir"], lengths=full["read_length"])
    rm.same(got, rm.realign([0, 1, 1, 2, 2], [2, 0], [0, 1], reads, full["qual"], band=62, density=0.01, min_minimizers=10))
    for h in (r, thin, m, rd):
        h.free()


# ---- pairs whose lengths are exact ----------------------------------------------------------------------------------------------------------
class Pool:
    """distinct values that stay at DENSITY, and distinct ones that go"""

    def __init__(self, seed: int, n: int):
        v = np.unique(np.random.default_rng(seed).integers(1, 1 << 32, 3 * n, dtype=np.uint64).astype(np.uint32))
        np.random.default_rng(seed + 1).shuffle(v)
        keep = rm.thin_keep(v, DENSITY)
        self.stay, self.go, self.rng = list(v[keep]), list(v[~keep]), np.random.default_rng(seed + 2)

    def take(self, n: int) -> list:
        out, self.stay = self.stay[:n], self.stay[n:]
        assert len(out) == n
        return [int(x) for x in out]


def read_of(pool: Pool, kept: list, positions=None, reverse=False) -> tuple:
    """a read whose thinned form is `kept` at `positions` (100 apart by default), a value that goes behind every one, the strand a value's
    lowest bit (equal values, equal strands), random qualities; reverse: stored reverse-complemented, so that the flag 1 gives it back"""
    n = len(kept)
    pos = np.arange(n, dtype=np.int64) * 100 + 50 if positions is None else np.asarray(positions, np.int64)
    m, p = [], []
    for k in range(n):
        m += [kept[k], int(pool.go.pop())]
        p += [int(pos[k]), int(pos[k]) + 1]
    m, p = np.array(m, np.uint32), np.array(p, np.int64)
    d = (m & 1).astype(np.uint8)
    q = pool.rng.integers(1, 41, len(m)).astype(np.uint8)
    length = (int(pos[-1]) if n else 0) + 60
    if reverse:
        m, p, d, q = m[::-1], length - p[::-1], (1 - d[::-1]).astype(np.uint8), q[::-1]
    return m, p.astype(np.uint32), d, length, q


def with_indels(pool: Pool, n_t: int, n_extra: int, n_missing: int) -> tuple:
    """T' of n_t values, at every planted place two equal ones side by side, and N' = T' but for the first of the two missing (n_missing
    places) or one copy more 50 bases in front of them (n_extra places): the chain runs along the equal positions, the raw list has
    n_t + n_extra entries, and normalisation moves an index at every missing place and two, the second a cascade, at every extra one"""
    t = pool.take(n_t)
    tp = list(range(50, 50 + 100 * n_t, 100))
    places = [20 + 37 * k for k in range(n_extra + n_missing)]
    assert places[-1] + 2 < n_t
    for at in places:
        t[at + 1] = t[at]
    missing, extra = set(places[:n_missing]), set(places[n_missing:])
    n, np_ = [], []
    for i in range(n_t):
        if i in missing:
            continue
        if i in extra:
            n.append(t[i]); np_.append(tp[i] - 50)
        n.append(t[i]); np_.append(tp[i])
    return (t, tp), (n, np_)


def built_pairs(L: int) -> dict:
    """Every built pair for ONE call: target 2 k, neighbour 2 k + 1, flag as listed; the row of every named pair"""
    pool = Pool(77, 30000)
    pairs, names = [], []

    def add(name, t, n, flag=0):
        names.append(name); pairs.append((t, n, flag))

    for raw in (L - 1, L, L + 1):                          # the lists' LDS seam, normalisation firing on both paths
        (t, tp), (n, np_) = with_indels(pool, raw - 3, 3, 2)
        add(f"raw{raw}", read_of(pool, t, tp), read_of(pool, n, np_))
    for links in (63, 64, 65):                             # the wave's trip over the links
        t = pool.take(links + 1)
        add(f"links{links}", read_of(pool, t), read_of(pool, t))
    for n_q in (9, 10, 11):                                # Utils::isReadTooShort
        t = pool.take(n_q)
        add(f"short{n_q}", read_of(pool, t), read_of(pool, t))
    for n_q in (1023, 1024, 1025):                         # the join's LDS seam under reversal, one value three times: the mirrored run
        t = pool.take(n_q)
        t[500] = t[700] = t[300]
        add(f"mirror{n_q}", read_of(pool, t), read_of(pool, t, reverse=True), 1)
    t = pool.take(16)                                      # the cascade: a run of one value, one copy more in the neighbour, the chain stepping over it
    t[7] = t[8] = t[6]
    tp = list(range(50, 1650, 100))
    n, np_ = t[:7] + [t[6]] + t[7:], tp[:7] + [tp[6] + 50] + tp[7:]
    add("cascade", read_of(pool, t, tp), read_of(pool, n, np_))
    t = pool.take(40)                                      # a wrong flag: the chain comes out reversed
    add("wrong_flag", read_of(pool, t), read_of(pool, t), 1)
    gone = np.array([pool.go.pop() for _ in range(5)], np.uint32)          # a target whose thinned form is empty: every value goes
    add("empty_target", (gone, np.arange(5, dtype=np.uint32) * 10 + 3, (gone & 1).astype(np.uint8), 100, np.full(5, 7, np.uint8)), read_of(pool, pool.take(12)))
    reads, quals = pack([r for t, n, _ in pairs for r in (t, n)])
    n_pairs = len(pairs)
    # target 2 k lists neighbour 2 k + 1; the last pair's neighbour, a target itself, lists nothing; one target more lists a read that is not there
    ko = np.zeros(2 * n_pairs + 2, np.uint64)
    ko[1::2][:n_pairs] = np.arange(1, n_pairs + 1)
    ko[2::2][:n_pairs] = np.arange(1, n_pairs + 1)
    ko[-1] = n_pairs + 1
    kn = np.concatenate([np.arange(1, 2 * n_pairs, 2), [5000]]).astype(np.uint32)
    kr = np.array([f for _, _, f in pairs] + [0], np.uint8)
    return dict(row={name: k for k, name in enumerate(names)}, reads=reads, quals=quals, kept=(ko, kn, kr), params=dict(band=62, density=DENSITY, min_minimizers=10), L=L)


@pytest.fixture(scope="module")
def built(ctx):
    """... on the device and by the model, with the model's per-row statistics"""
    L = ctx.realign_lds_entries()
    assert L == 1024
    b = built_pairs(L)
    got, info = device_pairs(ctx, *b["kept"], b["reads"], b["quals"], **b["params"])
    stats = {}
    want = rm.realign(*b["kept"], b["reads"], b["quals"], stats=stats, **b["params"])
    return dict(b, got=got, info=info, want=want, stats=stats)


def test_built_pairs_equal_the_model(built):
    rm.same(built["got"], built["want"])
    assert built["info"] == rm.info(built["want"])


def test_list_lengths_at_the_lds_seam(built):
    L, rows, stats = built["L"], built["got"]["rows"], built["stats"]["rows"]
    for raw in (L - 1, L, L + 1):
        s = built["row"][f"raw{raw}"]
        assert rows["flags"][s] == rm.REALIGN_CHAIN and stats[s]["raw"] == raw and stats[s]["moves"] >= 5
        assert rows["n_deletions"][s] == 2 and rows["n_insertions"][s] == 3 and rows["n_entries"][s] == raw - stats[s].get("erased", 0)


def test_chains_at_the_waves_trip(built):
    rows = built["got"]["rows"]
    for links in (63, 64, 65):
        s = built["row"][f"links{links}"]
        assert rows["flags"][s] == rm.REALIGN_CHAIN and rows["n_matches"][s] == links + 1 == rows["n_entries"][s]
        e = built["got"]["entry_offsets"].astype(np.int64)
        assert np.array_equal(built["got"]["ref_index"][e[s]:e[s + 1]], np.arange(links + 1)) and not built["got"]["kind"][e[s]:e[s + 1]].any()


def test_neighbours_at_the_shortest_length(built):
    rows = built["got"]["rows"]
    assert [int(rows["flags"][built["row"][f"short{n}"]]) for n in (9, 10, 11)] == [rm.REALIGN_SHORT, rm.REALIGN_CHAIN, rm.REALIGN_CHAIN]
    short = rows[built["row"]["short9"]]
    assert all(int(short[f]) == 0 for f in rm.REALIGNED.names if f not in ("neighbour", "flags"))


def test_reversed_neighbours_at_the_joins_lds_seam(built):
    rows, got = built["got"]["rows"], built["got"]
    e = got["entry_offsets"].astype(np.int64)
    for n_q in (1023, 1024, 1025):
        s = built["row"][f"mirror{n_q}"]
        assert rows["flags"][s] == rm.REALIGN_CHAIN and rows["oriented_reversed"][s] == 1 and rows["chain_reversed"][s] == 0
        assert rows["n_anchors"][s] == n_q + 6 and rows["n_matches"][s] == n_q == rows["n_entries"][s]
        assert np.array_equal(got["query_index"][e[s]:e[s + 1]], np.arange(n_q)) and not got["kind"][e[s]:e[s + 1]].any()
        t0 = int(got["target_offsets"][2 * s])
        assert np.array_equal(got["query_minimizer"][e[s]:e[s + 1]], got["target_minimizer"][t0:t0 + n_q])


def test_the_cascade_and_a_wrong_flag(built):
    rows, stats = built["got"]["rows"], built["stats"]["rows"]
    s = built["row"]["cascade"]
    assert stats[s]["cascades"] >= 1 and stats[s]["raw"] == 17 and rows["n_insertions"][s] == 1
    e = built["got"]["entry_offsets"].astype(np.int64)
    assert [int(k) for k in built["got"]["kind"][e[s]:e[s + 1]]] == [0] * 9 + [rm.INSERTION] + [0] * 7       # the insertion has moved to the end of the run
    w = built["row"]["wrong_flag"]
    assert rows["flags"][w] == rm.REALIGN_CHAIN and rows["chain_reversed"][w] == 1 and rows["oriented_reversed"][w] == 1


def test_targets_without_rows_empty_and_absent(built):
    got, rows = built["got"], built["got"]["rows"]
    n_pairs = len(built["row"])
    to = got["target_offsets"].astype(np.int64)
    s = built["row"]["empty_target"]
    assert to[2 * s + 1] == to[2 * s] and rows["flags"][s] == 0 and rows["n_anchors"][s] == 0          # T' is empty: no anchors, no chain
    assert to[2 * s + 2] - to[2 * s + 1] == 12 and got["row_offsets"][2 * s + 2] == got["row_offsets"][2 * s + 1]      # a target with no kept row has its backbone
    assert rows["flags"][n_pairs] == rm.REALIGN_ABSENT and rows["neighbour"][n_pairs] == 5000 and to[-1] == to[-2]      # the target behind the reads
    assert all(int(rows[n_pairs][f]) == 0 for f in rm.REALIGNED.names if f not in ("neighbour", "flags"))


def test_a_set_without_qualities_and_two_ranges(ctx, built):
    ko, kn, kr = built["kept"]
    got, _ = device_pairs(ctx, ko, kn, kr, built["reads"], None, **built["params"])
    assert not got["query_quality"].any() and not got["target_quality"].any() and built["got"]["query_quality"].any()
    for k in got:
        if k not in ("query_quality", "target_quality"):
            assert np.array_equal(got[k], built["got"][k]), k
    # the reads from read 6 on as their own set: the rows of the first three pairs are absent, the others as before
    off = built["reads"]["offsets"].astype(np.int64)
    part = dict(offsets=(off[6:] - off[6]).astype(np.uint64), lengths=built["reads"]["lengths"][6:], **{k: built["reads"][k][off[6]:] for k in ("minimizers", "positions", "directions")})
    got, _ = device_pairs(ctx, ko, kn, kr, part, built["quals"][off[6]:], reads_first_read=6, **built["params"])
    rm.same(got, rm.realign(ko, kn, kr, part, built["quals"][off[6]:], reads_first_read=6, **built["params"]))
    assert [int(f) for f in got["rows"]["flags"][:4]] == [rm.REALIGN_ABSENT] * 3 + [rm.REALIGN_CHAIN] and np.array_equal(got["rows"][3:-1], built["got"]["rows"][3:-1])


# ---- qualities attached, refusals, empty inputs, timers, two contexts ---------------------------------------------------------------------------
def test_attach_qualities_round_trip_and_refusals(ctx):
    from metamdbg_amd import capi
    pool = Pool(5, 200)
    reads, quals = pack([read_of(pool, pool.take(12)), read_of(pool, pool.take(15))])
    bare = ctx.minimizers_from_host(reads["minimizers"], reads["offsets"])
    with pytest.raises(capi.MdbgError, match="no positions") as e:
        bare.attach_qualities(quals)
    assert e.value.code == -1
    bare.attach_positions(reads["positions"])
    bare.attach_qualities(quals)                                                        # (before the strands: positions are all it asks for)
    with pytest.raises(capi.MdbgError, match="directions and read lengths"):
        ctx.map_realign_pairs([0, 1, 1], [1], [0], bare)
    bare.attach_strands(reads["directions"], reads["lengths"])
    r = ctx.map_realign_pairs([0, 0, 0], [], [], bare, 0, 0, 62, 1.0, 10)               # density 1: the backbone is the reads, the qualities those attached
    got = r.to_host()
    assert np.array_equal(got["target_offsets"], reads["offsets"]) and np.array_equal(got["target_minimizer"], reads["minimizers"]) and np.array_equal(got["target_quality"], quals)
    r.free()
    rd = ctx.reads_from_ascii([b"ACGTTGCAAGGCTTAACCGGTTAGCATCGATCGGATCCATGCAT" * 4])
    scanned = ctx.scan(rd, K=15, density=0.2, hpc=False, apply_read_filters=False)
    n = scanned.info()["n_minimizers"]
    with pytest.raises(capi.MdbgError, match="a scan output has its qualities"):
        scanned.attach_qualities(np.zeros(n, np.uint8))
    for h in (scanned, rd, bare):
        h.free()


def test_refusals(ctx):
    from metamdbg_amd import capi
    pool = Pool(6, 200)
    t = pool.take(12)
    reads, quals = pack([read_of(pool, t), read_of(pool, t)])
    m = upload(ctx, reads, quals)
    good = ([0, 1, 1], [1], [0], m, 0, 0)
    for args, match in (((0, DENSITY, 10), "max_chaining_band is 0"), ((62, 0.0, 10), "assembly_density must be > 0"), ((62, float("nan"), 10), "assembly_density must be > 0"),
                        ((62, DENSITY, 0), "min_minimizers is 0")):
        with pytest.raises(capi.MdbgError, match=match) as e:
            ctx.map_realign_pairs(*good, *args)
        assert e.value.code == -1
    with pytest.raises(capi.MdbgError, match="kept_offsets"):
        ctx.map_realign_pairs([0, 1, 0], [1], [0], m)
    with pytest.raises(capi.MdbgError, match="kept_offsets"):
        ctx.map_realign_pairs([1, 1, 1], [1], [0], m)
    with pytest.raises(capi.MdbgError, match="neither 0 nor 1"):
        ctx.map_realign_pairs([0, 1, 1], [1], [2], m)
    with pytest.raises(capi.MdbgError, match="null argument"):
        ctx.map_realign_pairs([0, 1, 1], [1], [0], None)
    with pytest.raises(capi.MdbgError, match="null argument"):
        ctx.map_realign(None, m)
    piece = ctx.minimizers_slice(m, 0, 1)
    with pytest.raises(capi.MdbgError, match="no positions"):
        ctx.map_realign_pairs([0, 0], [], [], piece)
    r = ctx.map_realign_pairs(*good, 62, DENSITY, 10)                                    # ... and the same objects are good for a call
    assert r.info() == dict(n_targets=2, n_rows=1, n_chains=1, n_entries=12)
    for h in (r, piece, m):
        h.free()


def test_empty_inputs(ctx):
    pool = Pool(7, 100)
    reads, quals = pack([read_of(pool, pool.take(12))])
    got, info = device_pairs(ctx, [0], [], [], reads, quals, band=62, density=DENSITY, min_minimizers=10)
    assert info == dict(n_targets=0, n_rows=0, n_chains=0, n_entries=0)
    assert np.array_equal(got["row_offsets"], [0]) and np.array_equal(got["entry_offsets"], [0]) and np.array_equal(got["target_offsets"], [0])
    assert all(len(got[k]) == 0 for k in ("rows", "ref_index", "query_index", "query_minimizer", "query_quality", "kind", "target_minimizer", "target_quality"))
    got, info = device_pairs(ctx, [0, 0, 0], [], [], reads, quals, band=62, density=DENSITY, min_minimizers=10)      # two targets, no rows: the backbone alone
    assert info == dict(n_targets=2, n_rows=0, n_chains=0, n_entries=0) and np.array_equal(got["target_offsets"], [0, 12, 12]) and np.array_equal(got["entry_offsets"], [0])


def test_timers_and_kernel_attributes(ctx):
    cfg = CONFIGS[1]
    d = rm.load_fixture(cfg["name"])
    m = upload(ctx, vm.fixture_reads(d), d["qualities"])
    ctx.timing(True)
    ctx.timing_reset()
    try:
        r = ctx.map_realign_pairs(d["kept_offsets"], d["kept_neighbour"], d["kept_reversed"], m, 0, 0, cfg["band"], cfg["density"], cfg["min_minimizers"])
        ctx.synchronize()
        counts = {name: ctx.timing_get(name)[1] for name in ("realign_thin", "realign_join", "realign_chains", "realign_lists", "radix_sort")}
    finally:
        ctx.timing(False)
    # thin: the flag; offsets + compaction; the backbone's count + scan; its gather.  join: the keys; sorted; the rows' reads + count + scan; fill.
    # lists: fill + normalise + scan; compaction.
    assert counts == dict(realign_thin=4, realign_join=4, realign_chains=1, realign_lists=2, radix_sort=1), counts
    assert r.info()["n_chains"] == cfg["chains"]
    r.free(); m.free()
    names = [n for n in ctx.step_kernel_names() if n.startswith("realign")]
    assert sorted(names) == sorted(["realign_join_fill", "realign_row_reads", "realign_backbone_count", "realign_backbone_gather", "realign_chain", "realign_lists",
                                    "realign_compact"])
    lds = 4 * 8 * ctx.realign_lds_entries()          # four waves a block, REALIGN_LDS_ENTRIES entries of two 32-bit indexes each
    assert lds == 32768 == 4 * 2 * 4 * ctx.verify_lds_anchors()
    for name in names:
        a = ctx.kernel_attributes(name)
        assert a["scratch"] == 0 and a["role"] == 2 and a["threads"] == 256 and a["static_lds"] == (lds if name in ("realign_join_fill", "realign_chain", "realign_lists") else 0), (name, a)


def test_two_contexts_on_two_threads(ctx):
    from metamdbg_amd import capi
    cfg = CONFIGS[0]
    d = rm.load_fixture(cfg["name"])
    m = upload(ctx, vm.fixture_reads(d), d["qualities"])
    other = capi.Context(0)
    out = {}

    def run(name, c):
        r = c.map_realign_pairs(d["kept_offsets"], d["kept_neighbour"], d["kept_reversed"], m, 0, 0, cfg["band"], cfg["density"], cfg["min_minimizers"])
        out[name] = r.to_host()
        r.free()

    threads = [threading.Thread(target=run, args=(k, c)) for k, c in (("a", ctx), ("b", other))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    rm.same(out["a"], out["b"])
    rm.same_as_fixture(out["a"], rm.fixture_realignment(d))
    m.free(); other.close()
