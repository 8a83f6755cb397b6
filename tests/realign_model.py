"""numpy restatement of mdbg_map_realign (metamdbg_amd/csrc/realign.hip, realign_dev.hpp), written from the first half of
ReadCorrectionFunctor::performPoaCorrection4 (ReadCorrection.hpp:5217-5285), Utils::getLowDensityMinimizerRead (Commons.hpp:2507-2574),
MinimizerRead::toReverseComplement (Commons.hpp:1042-1079) and MinimizerChainer::computeChainingAlignment / normalizeAlignment
(MinimizerChainer.hpp:330-569, :1015-1111).  The anchors of a pair and the chain are tests/verify_model.py's.
tests/test_read_realign_model.py holds it against the reference's own output (tests/golden/read_realign); the GPU tests use it on inputs the
fixture does not have.  The layouts are those of capi.Realignment.to_host().

T' is the thinned target, N' the thinned neighbour as oriented; an entry is (ref_index, query_index), NONE for the reference's -1.  The list
is kept as a python list and normalised with `del`, as the reference erases: nothing here knows of tombstones."""
from __future__ import annotations

import json
import os

import numpy as np

from tests import verify_model as vm

REALIGN_CHAIN, REALIGN_ABSENT, REALIGN_TOO_LONG, REALIGN_SHORT = 1, 4, 8, 16
MATCH, MISMATCH, INSERTION, DELETION = 0, 1, 2, 3
NONE = 0xFFFFFFFF
REALIGNED = np.dtype([("neighbour", "<u4"), ("flags", "<u4"), ("oriented_reversed", "<u4"), ("chain_reversed", "<u4"), ("n_anchors", "<u4"), ("n_entries", "<u4"),
                      ("n_matches", "<i4"), ("n_mismatches", "<i4"), ("n_deletions", "<i4"), ("n_insertions", "<i4"),
                      ("reference_start_index", "<u4"), ("reference_end_index", "<u4")])
ENTRY_ARRAYS = ("ref_index", "query_index", "query_minimizer", "query_quality", "kind")
DEFAULTS = dict(band=62, density=0.005, min_minimizers=10)

FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "read_realign")


# ---- the density rule (Commons.hpp:2520-2531): Murmur3_x64_128 of the value as 8 bytes, seed 42, its first half below density * 2^64 ---------
def _fmix(k):
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xff51afd7ed558ccd)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xc4ceb9fe1a85ec53)
    return k ^ (k >> np.uint64(33))


def kmer_hash(values) -> np.ndarray:
    with np.errstate(over="ignore"):
        k = np.asarray(values).astype(np.uint64) * np.uint64(0x87c37b91114253d5)
        k = ((k << np.uint64(31)) | (k >> np.uint64(33))) * np.uint64(0x4cf5ad432745937f)
        h1 = ((np.uint64(42) ^ k) ^ np.uint64(8)) + (np.uint64(42) ^ np.uint64(8))        # h1 ^= len; h2 ^= len; h1 += h2
        h2 = h1 + (np.uint64(42) ^ np.uint64(8))                                          # h2 += h1
        return _fmix(h1) + _fmix(h2)


def thin_keep(minimizers, density: float) -> np.ndarray:
    """True where the reference's thinning keeps the minimizer: the u64 hash compared as a double with the float density times 2^64 - 1 as a double."""
    bound = np.float64(np.float32(density)) * np.float64(0xFFFFFFFFFFFFFFFF)
    return kmer_hash(minimizers).astype(np.float64) < bound


# ---- one pair -------------------------------------------------------------------------------------------------------------------------------
def oriented(m, p, d, q, length: int, reversed_: bool):
    """toReverseComplement: the order turned round, then dir = !dir, pos = length - pos."""
    if not reversed_:
        return m, p, d, q
    return m[::-1], (length - p[::-1].astype(np.int64)).astype(np.uint32), (1 - d[::-1]).astype(np.uint8), q[::-1]


def raw_list(walk, an, n_t: int, n_q: int):
    """_alignments before normalisation (:330-569) with the reference's two running counters, and AlignmentResult2's counts."""
    ri, qi = [int(x) for x in an["ri"]], [int(x) for x in an["qi"]]
    f, l = walk[0], walk[-1]
    rev = qi[f] > qi[l]
    step = -1 if rev else 1
    if rev:
        start_mis, end_mis = min(ri[f], n_q - qi[f] - 1), min(n_t - ri[l] - 1, qi[l])
    else:
        start_mis, end_mis = min(ri[f], qi[f]), min(n_t - ri[l] - 1, n_q - qi[l] - 1)
    r, q = ri[f] - start_mis, qi[f] - step * start_mis
    out = []
    n_mis, n_del, n_ins = start_mis + end_mis, 0, 0
    for _ in range(start_mis):
        out.append([r, q]); r += 1; q += step
    for a, b in zip(walk[:-1], walk[1:]):
        rg = ri[b] - ri[a] - 1
        qg = (qi[a] - qi[b] if rev else qi[b] - qi[a]) - 1
        mis = min(rg, qg)
        dele, ins = (rg - mis, 0) if rg > qg else (0, qg - mis)
        assert (r, q) == (ri[a], qi[a])
        out.append([r, q]); r += 1; q += step
        for _ in range(mis + dele):
            out.append([r, NONE]); r += 1
        for _ in range(mis + ins):
            out.append([NONE, q]); q += step
        n_mis += mis; n_del += dele; n_ins += ins
    assert (r, q) == (ri[l], qi[l])
    out.append([r, q]); r += 1; q += step
    for _ in range(end_mis):
        out.append([r, q]); r += 1; q += step
    return out, dict(chain_reversed=int(rev), n_matches=len(walk), n_mismatches=n_mis, n_deletions=n_del, n_insertions=n_ins, reference_start_index=ri[f],
                     reference_end_index=ri[l])


def normalize(lst, tm, qm, stats=None):
    """normalizeAlignment (:1015-1111): one forward pass, in-place edits, erase.  stats counts the moves, the erased entries and the cascades
    (an entry that lost an index to an earlier one takes one itself)."""
    bump = lambda k: stats.__setitem__(k, stats.get(k, 0) + 1) if stats is not None else None
    robbed = [False] * len(lst)
    i = 0
    while i < len(lst):
        r, q = lst[i]
        side = 0 if r == NONE else 1 if q == NONE else None
        if side is not None:
            j = next((j for j in range(i, len(lst)) if lst[j][side] != NONE), None)
            if j is not None:
                if (tm[lst[j][0]] == qm[q]) if side == 0 else (tm[r] == qm[lst[j][1]]):
                    lst[i][side] = lst[j][side]; lst[j][side] = NONE
                    bump("moves")
                    if robbed[i]:
                        bump("cascades")
                    robbed[j] = True
                if lst[j] == [NONE, NONE]:
                    del lst[j], robbed[j]
                    bump("erased")
        i += 1
    return lst


def kinds(lst, tm, qm) -> list:
    return [INSERTION if r == NONE else DELETION if q == NONE else MATCH if tm[r] == qm[q] else MISMATCH for r, q in lst]


# ---- a whole call ---------------------------------------------------------------------------------------------------------------------------
def realign(kept_offsets, kept_neighbour, kept_reversed, reads: dict, qualities=None, target_first_read=0, reads_first_read=0, band=62, density=0.005, min_minimizers=10,
            stats=None) -> dict:
    """reads: dict(offsets, minimizers, positions, directions, lengths); qualities: one byte per minimizer or None (zeros)."""
    off = np.asarray(reads["offsets"], np.int64)
    n_reads = len(off) - 1
    qual = np.zeros(int(off[-1]), np.uint8) if qualities is None else np.asarray(qualities, np.uint8)
    keep = thin_keep(reads["minimizers"], density)

    def thinned(r):
        k = keep[off[r]:off[r + 1]]
        piece = lambda a: np.asarray(a)[off[r]:off[r + 1]][k]
        return piece(reads["minimizers"]), piece(reads["positions"]), piece(reads["directions"]), piece(qual)

    ko = np.asarray(kept_offsets, np.int64)
    n_targets, n_rows = len(ko) - 1, int(ko[-1])
    rows = np.zeros(n_rows, REALIGNED)
    rows["neighbour"] = np.asarray(kept_neighbour, np.uint32)
    entry_offsets = np.zeros(n_rows + 1, np.uint64)
    cols = {k: [] for k in ENTRY_ARRAYS}
    target_offsets = np.zeros(n_targets + 1, np.uint64)
    tmin, tqual = [], []
    for t in range(n_targets):
        tl = target_first_read + t - reads_first_read
        present = 0 <= tl < n_reads
        if present:
            tm, tp, td, tq = thinned(tl)
            tmin.append(tm); tqual.append(tq)
        target_offsets[t + 1] = target_offsets[t] + (len(tm) if present else 0)
        for s in range(int(ko[t]), int(ko[t + 1])):
            entry_offsets[s + 1] = entry_offsets[s]
            ql = int(rows["neighbour"][s]) - reads_first_read
            if not (present and 0 <= ql < n_reads):
                rows["flags"][s] = REALIGN_ABSENT
                continue
            qm, qp, qd, qq = thinned(ql)
            if len(qm) < min_minimizers:
                rows["flags"][s] = REALIGN_SHORT
                continue
            flag = bool(kept_reversed[s])
            qm, qp, qd, qq = oriented(qm, qp, qd, qq, int(reads["lengths"][ql]), flag)
            an = vm.pair_anchors(tm, tp, td, qm, qp, qd)
            n = len(an["ri"])
            if n >= vm.TOO_LONG_FROM:
                rows["flags"][s] = REALIGN_TOO_LONG
                continue
            rows["oriented_reversed"][s] = flag
            rows["n_anchors"][s] = n
            if n < vm.MIN_ANCHORS:
                continue
            walk = vm.chain_walk(an["rpos"], an["qpos"], an["rev"], band)
            if len(walk) < vm.MIN_CHAIN:
                continue
            lst, fields = raw_list(walk, an, len(tm), len(qm))
            mine = dict(raw=len(lst))                  # per row: the raw length, and what normalisation did
            lst = normalize(lst, tm, qm, mine)
            if stats is not None:
                stats.setdefault("rows", {})[s] = mine
                for k in ("moves", "erased", "cascades"):
                    stats[k] = stats.get(k, 0) + mine.get(k, 0)
            for k, v in fields.items():
                rows[k][s] = v
            rows["flags"][s] = REALIGN_CHAIN
            rows["n_entries"][s] = len(lst)
            entry_offsets[s + 1] = entry_offsets[s] + len(lst)
            cols["ref_index"] += [r for r, _ in lst]
            cols["query_index"] += [q for _, q in lst]
            cols["query_minimizer"] += [0 if q == NONE else int(qm[q]) for _, q in lst]
            cols["query_quality"] += [0 if q == NONE else int(qq[q]) for _, q in lst]
            cols["kind"] += kinds(lst, tm, qm)
    cat = lambda parts, t: np.concatenate(parts).astype(t) if parts else np.zeros(0, t)
    return dict(row_offsets=ko.astype(np.uint64), rows=rows, entry_offsets=entry_offsets, ref_index=np.array(cols["ref_index"], np.uint32),
                query_index=np.array(cols["query_index"], np.uint32), query_minimizer=np.array(cols["query_minimizer"], np.uint32),
                query_quality=np.array(cols["query_quality"], np.uint8), kind=np.array(cols["kind"], np.uint8), target_offsets=target_offsets,
                target_minimizer=cat(tmin, np.uint32), target_quality=cat(tqual, np.uint8))


def info(r: dict) -> dict:
    return dict(n_targets=len(r["row_offsets"]) - 1, n_rows=len(r["rows"]), n_chains=int(((r["rows"]["flags"] & REALIGN_CHAIN) != 0).sum()), n_entries=len(r["ref_index"]))


def same(a: dict, b: dict) -> None:
    assert sorted(a) == sorted(b)
    for f in REALIGNED.names:
        bad = np.flatnonzero(a["rows"][f] != b["rows"][f])
        assert len(bad) == 0, (f, bad[:5], a["rows"][bad[:5]], b["rows"][bad[:5]])
    for k in a:
        if k != "rows":
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (k, len(a[k]), len(b[k]), np.flatnonzero(a[k][:min(len(a[k]), len(b[k]))] != b[k][:min(len(a[k]), len(b[k]))])[:5])


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------------
def fixture_manifest() -> dict:
    with open(os.path.join(FIXTURE_DIR, "manifest.json")) as f:
        return json.load(f)


def load_fixture(name: str) -> dict:
    """tests/golden/read_realign/<name>.npz, its delta-coded arrays summed up again; the reads are those of the read_verify file the manifest
    names under reads_from (the same generator, the same seed) unless the file carries its own."""
    man = fixture_manifest()
    cfg = next(c for c in man["configs"] if c["name"] == name)
    delta = set(man["delta_coded"])
    with np.load(os.path.join(FIXTURE_DIR, name + ".npz")) as z:
        d = {k: (np.cumsum(z[k].astype(np.int64)).astype(np.uint32) if k in delta else z[k]) for k in z.files}
    if cfg.get("reads_from"):
        v = vm.load_fixture(cfg["reads_from"])
        for k in ("read_offsets", "minimizers", "positions", "directions", "read_lengths"):
            d[k] = v[k]
    return d


def fixture_params(cfg: dict) -> dict:
    return dict(band=cfg["band"], density=cfg["density"], min_minimizers=cfg["min_minimizers"])


def query_checksum(r: dict) -> np.ndarray:
    """Per row the sum over its entries k = 0, 1, ... that have a query_index of (k + 1) * query_minimizer, mod 2^32 (what the fixture holds of the
    entries' minimizers: they would not fit its size)."""
    eo = r["entry_offsets"].astype(np.int64)
    out = np.zeros(len(eo) - 1, np.uint32)
    for s in range(len(out)):
        m = r["query_minimizer"][eo[s]:eo[s + 1]].astype(np.uint64)
        has = r["query_index"][eo[s]:eo[s + 1]] != NONE
        out[s] = int(((np.arange(1, len(m) + 1, dtype=np.uint64) * m)[has]).sum()) & 0xFFFFFFFF
    return out


def fixture_realignment(d: dict) -> dict:
    """The REFERENCE's rows and lists of a fixture file in the layout of capi.Realignment.to_host() -- but for query_minimizer, of which the
    fixture holds row_query_checksum (query_checksum above); the backbone from the reference's own thinning (thin_index)."""
    n = len(d["kept_neighbour"])
    rows = np.zeros(n, REALIGNED)
    rows["neighbour"] = d["kept_neighbour"]
    state = d["row_state"].astype(np.uint32)
    rows["flags"] = state
    rows["oriented_reversed"] = np.where(state != REALIGN_SHORT, d["kept_reversed"], 0)
    for k in ("chain_reversed", "n_anchors", "n_entries", "n_matches", "n_mismatches", "n_deletions", "n_insertions", "reference_start_index", "reference_end_index"):
        rows[k] = d["row_" + k]
    off = d["read_offsets"].astype(np.int64)
    keep = np.zeros(int(off[-1]), bool)
    keep[d["thin_index"]] = True
    ko = d["kept_offsets"].astype(np.int64)
    n_targets = len(ko) - 1
    cut = np.arange(off[0], off[n_targets])              # target t is read t
    cut = cut[keep[cut]]
    counts = np.array([int(keep[off[t]:off[t + 1]].sum()) for t in range(n_targets)], np.int64)
    eo = np.concatenate([[0], np.cumsum(rows["n_entries"].astype(np.int64))]).astype(np.uint64)
    return dict(row_offsets=ko.astype(np.uint64), rows=rows, entry_offsets=eo, ref_index=d["entry_ref_index"].astype(np.uint32),
                query_index=d["entry_query_index"].astype(np.uint32), row_query_checksum=d["row_query_checksum"].astype(np.uint32),
                query_quality=d["entry_query_quality"].astype(np.uint8), kind=d["entry_kind"].astype(np.uint8),
                target_offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), target_minimizer=d["minimizers"][cut].astype(np.uint32),
                target_quality=d["qualities"][cut].astype(np.uint8))


def same_as_fixture(got: dict, ref: dict) -> None:
    """A result in to_host()'s layout against fixture_realignment's: every array, the minimizers by their checksum."""
    g = dict(got)
    g["row_query_checksum"] = query_checksum(got)
    del g["query_minimizer"]
    same(g, ref)
