"""mdbg_minimizers_attach_strands / mdbg_map_verify (csrc/verify.hip, verify_dev.hpp) on the device.

Against the REFERENCE: tests/golden/read_verify holds what MinimizerChainer::computeChainingAlignment and the four tests of
ReadCorrectionFunctor::filterAlignments computed for seeded reads at bands 62, 5 and 100 (verify_ref.cpp; tests/test_read_verify_model.py holds
the numpy model against the same files).  Every row and both kept arrays are compared for equality.

Against the model (tests/verify_model.py), on inputs the fixture does not have: the reads cut into two ranges, pairs whose anchors and whose
neighbour lengths sit at the 1 024 a wave keeps in LDS, a real scan output with its concat and thresholded forms (and a slice refused), a pair of 457 x 457 anchors and one too long to chain, refusals, empty inputs, two
contexts on two threads.

Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import threading

import numpy as np
import pytest

from tests import verify_model as vm

pytestmark = pytest.mark.gpu

CONFIGS = vm.fixture_manifest()["configs"]


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def upload(ctx, reads: dict):
    return ctx.minimizers_with_strands(reads["minimizers"], reads["offsets"], reads["positions"], reads["directions"], reads["lengths"])


def selection(ctx, sel_offsets, sel_neighbour):
    """a selection of these rows: every row's match list is the one position 0 (mdbg_map_verify reads the rows only)"""
    n = len(sel_neighbour)
    return ctx.selection_from_host(sel_offsets, sel_neighbour, np.arange(n + 1, dtype=np.uint64), np.zeros(n, np.uint32))


def device(ctx, sel_offsets, sel_neighbour, reads: dict, target_first_read=0, reads_first_read=0, **params) -> tuple:
    m, sel = upload(ctx, reads), selection(ctx, sel_offsets, sel_neighbour)
    v = ctx.map_verify(sel, m, target_first_read, reads_first_read, **params)
    out = v.to_host(), v.info()
    for h in (v, sel, m):
        h.free()
    return out


def pack(reads: list) -> dict:
    """[(minimizers, positions, directions, length), ...] -> the model's dict"""
    cat = lambda k, t: np.concatenate([np.asarray(r[k], t) for r in reads]) if reads else np.zeros(0, t)
    return dict(offsets=np.concatenate([[0], np.cumsum([len(r[0]) for r in reads])]).astype(np.uint64), minimizers=cat(0, np.uint32), positions=cat(1, np.uint32),
                directions=cat(2, np.uint8), lengths=np.array([r[3] for r in reads], np.uint32))


def repeated(value: int, n: int, step: int = 40) -> tuple:
    """a read of n copies of one minimizer, positions ascending"""
    return np.full(n, value, np.uint32), np.arange(n, dtype=np.uint32) * step + 7, np.zeros(n, np.uint8), n * step + 50


def pairs_selection(n_pairs: int) -> tuple:
    """target 2 k meets neighbour 2 k + 1; the odd reads list nothing"""
    off = np.zeros(2 * n_pairs + 1, np.uint64)
    off[1::2] = np.arange(1, n_pairs + 1)
    off[2::2] = np.arange(1, n_pairs + 1)
    return off, np.arange(1, 2 * n_pairs, 2, dtype=np.uint32)


# ---- the reference's fixture ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=CONFIGS, ids=[c["name"] for c in CONFIGS])
def case(request, ctx):
    cfg = request.param
    d = vm.load_fixture(cfg["name"])
    got, info = device(ctx, d["sel_offsets"], d["sel_neighbour"], vm.fixture_reads(d), **vm.fixture_params(cfg))
    return dict(cfg=cfg, d=d, got=got, info=info)


def test_rows_and_kept_lists_against_the_reference(case):
    cfg = case["cfg"]
    vm.same(case["got"], vm.fixture_verification(case["d"]))
    assert case["info"] == dict(n_targets=cfg["n_targets"], n_rows=cfg["rows"], n_chains=cfg["chains"], n_kept=cfg["kept"])
    assert cfg["kept"] >= 50 and cfg["chains"] > cfg["kept"]


def test_two_ranges_of_reads(ctx):
    cfg = CONFIGS[0]
    d = vm.load_fixture(cfg["name"])
    reads, whole = vm.fixture_reads(d), vm.fixture_verification(d)
    off = d["read_offsets"].astype(np.int64)
    n = len(off) - 1
    h = n // 2
    target = np.repeat(np.arange(n), np.diff(d["sel_offsets"].astype(np.int64)))
    seen = np.zeros(len(target), bool)
    for lo, hi in ((0, h), (h, n)):
        part = dict(offsets=(off[lo:hi + 1] - off[lo]).astype(np.uint64), lengths=reads["lengths"][lo:hi],
                    **{k: reads[k][off[lo]:off[hi]] for k in ("minimizers", "positions", "directions")})
        got, info = device(ctx, d["sel_offsets"], d["sel_neighbour"], part, 0, lo, **vm.fixture_params(cfg))
        vm.same(got, vm.verify(d["sel_offsets"], d["sel_neighbour"], part, 0, lo, **vm.fixture_params(cfg)))
        present = (target >= lo) & (target < hi) & (d["sel_neighbour"] >= lo) & (d["sel_neighbour"] < hi)
        assert np.array_equal((got["rows"]["flags"] & vm.VERIFY_ABSENT) != 0, ~present)
        assert np.array_equal(got["rows"][present], whole["rows"][present])
        zero = got["rows"][~present]
        assert all(not zero[f].any() for f in vm.VERIFIED.names if f not in ("neighbour", "flags"))
        keep = present & ((whole["rows"]["flags"] & vm.VERIFY_KEPT) != 0)
        assert np.array_equal(got["kept_neighbour"], d["sel_neighbour"][keep]) and np.array_equal(got["kept_reversed"], whole["rows"]["query_reversed"][keep])
        assert info["n_kept"] == int(keep.sum()) > 0
        seen |= present
    assert 0 < int(seen.sum()) < len(seen)


# ---- the seams of the LDS share ------------------------------------------------------------------------------------------------------------
def test_lds_seams(ctx):
    L = ctx.verify_lds_anchors()
    assert L == 1024
    shapes = [(33, 31), (32, 32), (41, 25),                  # L - 1, L and L + 1 anchors, a chain along the diagonal
              (1, L - 1), (1, L), (1, L + 1),                # the neighbour one below, at and one above the join's LDS capacity (and the same anchors)
              (L - 1, 1), (L + 1, 1),
              (4, L - 1), (4, L), (4, L + 1)]                # ... with a chain: the predecessor lies a whole neighbour back, inside the band of 1 100
    reads = []
    for k, (a, b) in enumerate(shapes):
        reads += [repeated(1000 + k, a), repeated(1000 + k, b)]
    reads = pack(reads)
    so, sn = pairs_selection(len(shapes))
    params = dict(band=1100, max_overhang=100000, min_overlap_length=100, min_identity=0.5, minimizer_size=15)
    got, info = device(ctx, so, sn, reads, **params)
    want = vm.verify(so, sn, reads, **params)
    vm.same(got, want)
    assert [int(x) for x in got["rows"]["n_anchors"]] == [a * b for a, b in shapes]
    chain = (got["rows"]["flags"] & vm.VERIFY_CHAIN) != 0
    assert [bool(c) for c in chain] == [min(a, b) >= 4 for a, b in shapes] and info["n_chains"] == 6
    assert [int(x) for x in got["rows"]["n_matches"][chain]] == [31, 32, 25, 4, 4, 4]


def test_pair_just_below_the_limit_and_one_too_long(ctx):
    """457 x 457 = 208 849 anchors are chained (scores and parents in global memory), 460 x 460 = 211 600 are refused.  The predecessor of
    grid anchor (i, j) is (i - 1, j - 1), 458 anchors back, so the band is 458.  The model's own dynamic programme over these anchors takes
    about six seconds, more than a case of this suite may; it returns the diagonal (vm.chain_walk(rpos, qpos, rev, 458) ==
    [458 k]), so here the chain is taken to be the diagonal -- which the model and the device confirm on a 40 x 40 grid at band 41 first --
    and the row is the model's summary of it."""
    small = pack([repeated(5, 40), repeated(5, 40)])
    so, sn = pairs_selection(1)
    params = dict(max_overhang=1000, min_overlap_length=1000, min_identity=0.96, minimizer_size=15)
    got, _ = device(ctx, so, sn, small, band=41, **params)
    want = vm.verify(so, sn, small, band=41, **params)
    vm.same(got, want)
    an = vm.pair_anchors(*[small[k][:40] for k in ("minimizers", "positions", "directions")] * 2)
    diagonal = vm.summary([k * 40 + k for k in range(40)], an, small["positions"][:40], small["positions"][40:], int(small["lengths"][0]), int(small["lengths"][1]))
    assert all(int(want["rows"][f][0]) == v for f, v in diagonal.items()) and want["rows"]["flags"][0] == vm.VERIFY_CHAIN | vm.VERIFY_KEPT

    n = 457
    reads = pack([repeated(9, n), repeated(9, n), repeated(11, 460), repeated(11, 460)])
    so, sn = pairs_selection(2)
    got, info = device(ctx, so, sn, reads, band=n + 1, **params)
    an = vm.pair_anchors(*[reads[k][:n] for k in ("minimizers", "positions", "directions")] * 2)
    assert len(an["ri"]) == 208849 < vm.TOO_LONG_FROM <= 460 * 460
    row = vm.summary([k * n + k for k in range(n)], an, reads["positions"][:n], reads["positions"][n:2 * n], int(reads["lengths"][0]), int(reads["lengths"][1]))
    first, second = got["rows"][0], got["rows"][1]
    assert first["n_anchors"] == 208849 and first["flags"] == vm.VERIFY_CHAIN | vm.VERIFY_KEPT and first["neighbour"] == 1
    assert {f: int(first[f]) for f in row} == row and row["n_matches"] == n
    assert second["flags"] == vm.VERIFY_TOO_LONG and second["neighbour"] == 3
    assert all(int(second[f]) == 0 for f in vm.VERIFIED.names if f not in ("neighbour", "flags"))
    assert info == dict(n_targets=4, n_rows=2, n_chains=1, n_kept=1)
    assert np.array_equal(got["kept_offsets"], [0, 1, 1, 1, 1]) and np.array_equal(got["kept_neighbour"], [1]) and np.array_equal(got["kept_reversed"], [0])


# ---- a scan output, its concat and its density-thresholded form; a slice carries values only --------------------------------------------------
def overlapping_reads(seed: int, n_reads: int = 14, genome: int = 24000) -> list:
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, genome)
    comp = np.array([3, 2, 1, 0])
    reads = []
    for _ in range(n_reads):
        n = int(rng.integers(5000, 9000))
        a = int(rng.integers(0, genome - n))
        r = g[a:a + n].copy()
        sub = rng.random(n) < 0.002
        r[sub] = rng.integers(0, 4, int(sub.sum()))
        if rng.random() < 0.5:
            r = comp[r[::-1]]
        reads.append(bytes(np.frombuffer(b"ACGT", np.uint8)[r]))
    return reads


def all_against_all(n: int) -> tuple:
    so = np.arange(n + 1, dtype=np.uint64) * np.uint64(n - 1)
    return so, np.concatenate([np.delete(np.arange(n, dtype=np.uint32), t) for t in range(n)])


def host_form(m) -> dict:
    h = m.to_host()
    return dict(offsets=h["offsets"], minimizers=h["minimizers"], positions=h["pos"], directions=h["dir"], lengths=h["read_length"])


def test_scan_output_its_concat_and_thresholded_form_and_what_a_slice_is(ctx):
    from metamdbg_amd import capi
    seqs = overlapping_reads(5)
    n = len(seqs)
    so, sn = all_against_all(n)
    sel = selection(ctx, so, sn)
    def scan(part):
        rd = ctx.reads_from_ascii(part)
        out = ctx.scan(rd, K=15, density=0.025, hpc=False, apply_read_filters=False)      # (positions and lengths in one coordinate system: both strands' pairs can pass the end overhang)
        rd.free()
        return out

    m = scan(seqs)
    v = ctx.map_verify(sel, m)                         # the fresh scan output, before anything else has read it
    got = v.to_host()
    v.free()
    reads = host_form(m)
    assert np.all(np.diff(reads["offsets"].astype(np.int64)) > 50) and set(np.unique(reads["directions"]).tolist()) == {0, 1}
    want = vm.verify(so, sn, reads)
    vm.same(got, want)
    assert len(want["kept_neighbour"]) >= 10 and 0 < int(want["kept_reversed"].sum()) < len(want["kept_reversed"])
    assert int(((want["rows"]["flags"] & vm.VERIFY_CHAIN) == 0).sum()) > 0
    # two scans one behind the other are the whole
    a, b = scan(seqs[:n // 2]), scan(seqs[n // 2:])
    both = ctx.minimizers_concat([a, b])
    v = ctx.map_verify(sel, both)
    vm.same(v.to_host(), want)
    v.free()
    # half the density: fewer minimizers, the same rules
    thin = ctx.apply_density_threshold(m, 0.0125)
    treads = host_form(thin)
    assert 0 < len(treads["minimizers"]) < len(reads["minimizers"])
    v = ctx.map_verify(sel, thin, band=31)
    vm.same(v.to_host(), vm.verify(so, sn, treads, band=31))
    v.free()
    # a slice carries offsets and values only: refused, not verified without its positions
    piece = ctx.minimizers_slice(m, 0, n // 2)
    with pytest.raises(capi.MdbgError, match="no positions") as e:
        ctx.map_verify(sel, piece)
    assert e.value.code == -1
    for h in (piece, thin, both, a, b, m, sel):
        h.free()


# ---- refusals, empty inputs ----------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from metamdbg_amd import capi
    reads = pack([repeated(5, 6), repeated(5, 6)])
    so, sn = pairs_selection(1)
    sel = selection(ctx, so, sn)
    bare = ctx.minimizers_from_host(reads["minimizers"], reads["offsets"])
    with pytest.raises(capi.MdbgError, match="no positions") as e:
        bare.attach_strands(reads["directions"], reads["lengths"])
    assert e.value.code == -1
    bare.attach_positions(reads["positions"])
    with pytest.raises(capi.MdbgError, match="directions and read lengths"):          # a set without strands
        ctx.map_verify(sel, bare)
    bad = reads["directions"].copy()
    bad[8] = 2
    with pytest.raises(capi.MdbgError, match=r"read 1, minimizer 2: direction 2"):
        bare.attach_strands(bad, reads["lengths"])
    bare.attach_strands(reads["directions"], reads["lengths"])
    with pytest.raises(capi.MdbgError, match="max_chaining_band is 0"):
        ctx.map_verify(sel, bare, band=0)
    with pytest.raises(capi.MdbgError, match="minimizer_size is 0"):
        ctx.map_verify(sel, bare, minimizer_size=0)
    with pytest.raises(capi.MdbgError, match="min_identity is not a number"):
        ctx.map_verify(sel, bare, min_identity=float("nan"))
    with pytest.raises(capi.MdbgError):
        ctx.verify_min_matches(10, float("nan"))
    v = ctx.map_verify(sel, bare)                                                     # ... and the same objects are good for a call
    assert v.info()["n_rows"] == 1 and v.to_host()["rows"]["n_anchors"][0] == 36
    for h in (v, bare, sel):
        h.free()


def test_empty_selection_and_targets_outside_the_reads(ctx):
    reads = pack([repeated(5, 6), repeated(5, 6)])
    got, info = device(ctx, np.zeros(3, np.uint64), np.zeros(0, np.uint32), reads)
    assert info == dict(n_targets=2, n_rows=0, n_chains=0, n_kept=0)
    assert np.array_equal(got["row_offsets"], [0, 0, 0]) and np.array_equal(got["kept_offsets"], [0, 0, 0]) and len(got["rows"]) == 0
    got, info = device(ctx, np.zeros(1, np.uint64), np.zeros(0, np.uint32), reads)
    assert info == dict(n_targets=0, n_rows=0, n_chains=0, n_kept=0)
    so, sn = pairs_selection(1)
    got, info = device(ctx, so, sn, reads, target_first_read=100)                      # targets 100 and 101: not among the reads 0 and 1
    assert info == dict(n_targets=2, n_rows=1, n_chains=0, n_kept=0)
    assert got["rows"]["flags"][0] == vm.VERIFY_ABSENT and got["rows"]["neighbour"][0] == 1 and got["rows"]["n_anchors"][0] == 0
    assert np.array_equal(got["kept_offsets"], [0, 0, 0]) and len(got["kept_neighbour"]) == 0


def test_timers_and_kernel_attributes(ctx):
    cfg = next(c for c in CONFIGS if c["name"] == "band5")
    d = vm.load_fixture("band5")
    m, sel = upload(ctx, vm.fixture_reads(d)), selection(ctx, d["sel_offsets"], d["sel_neighbour"])
    ctx.timing(True)
    ctx.timing_reset()
    try:
        v = ctx.map_verify(sel, m, **vm.fixture_params(cfg))
        ctx.synchronize()
        counts = {name: ctx.timing_get(name)[1] for name in ("verify_join", "verify_chains", "verify_rows", "radix_sort")}
    finally:
        ctx.timing(False)
    # join: the keys in front of the sort; sorted + longest read + the rows' reads + count + its scan; fill.  rows: the tests + scan; the kept rows.
    assert counts == dict(verify_join=3, verify_chains=1, verify_rows=2, radix_sort=1), counts
    assert v.info()["n_chains"] == cfg["chains"]
    for h in (v, sel, m):
        h.free()
    names = [n for n in ctx.step_kernel_names() if n.startswith("verify")]
    assert sorted(names) == sorted(["verify_keys", "verify_sorted", "verify_longest_read", "verify_row_reads", "verify_join_count", "verify_join_fill", "verify_chain",
                                    "verify_rows", "verify_kept"])
    # four waves a block, each with two arrays of 32-bit words, verify_lds_anchors long: scores and parents (chain), keys and indexes (join)
    wave_arrays = 4 * 2 * 4 * ctx.verify_lds_anchors()
    assert wave_arrays == 32768
    for name in names:
        a = ctx.kernel_attributes(name)
        lds = wave_arrays if name in ("verify_chain", "verify_join_count", "verify_join_fill") else 0
        assert a["scratch"] == 0 and a["role"] == 2 and a["threads"] == 256 and a["static_lds"] == lds, (name, a)


def test_two_contexts_on_two_threads(ctx):
    from metamdbg_amd import capi
    cfg = CONFIGS[0]
    d = vm.load_fixture(cfg["name"])
    m, sel = upload(ctx, vm.fixture_reads(d)), selection(ctx, d["sel_offsets"], d["sel_neighbour"])
    other = capi.Context(0)
    out = {}

    def run(name, c):
        v = c.map_verify(sel, m, **vm.fixture_params(cfg))
        out[name] = v.to_host()
        v.free()

    threads = [threading.Thread(target=run, args=(k, c)) for k, c in (("a", ctx), ("b", other))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    vm.same(out["a"], out["b"])
    vm.same(out["a"], vm.fixture_verification(d))
    sel.free(); m.free(); other.close()
