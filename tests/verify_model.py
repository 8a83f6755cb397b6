"""numpy restatement of mdbg_map_verify (metamdbg_amd/csrc/verify.hip, verify_dev.hpp), written from ReadCorrectionFunctor::filterAlignments
(ReadCorrection.hpp:5006-5117) and MinimizerChainer::computeChainingAlignment / chainAnchors / argmaxPosition (MinimizerChainer.hpp:114-961).
tests/test_read_verify_model.py holds it against the reference's own output (tests/golden/read_verify); the GPU tests use it on inputs the
fixture does not have.  The layouts are those of capi.Verification.to_host().

The TARGET is the read being corrected (the reference's referenceRead, a query of the selection), the NEIGHBOUR the other read."""
from __future__ import annotations

import json
import os

import numpy as np

VERIFY_CHAIN, VERIFY_KEPT, VERIFY_ABSENT, VERIFY_TOO_LONG = 1, 2, 4, 8
TOO_LONG_FROM = (1 << 24) // 80
MIN_ANCHORS, MIN_CHAIN = 3, 4
VERIFIED = np.dtype([("neighbour", "<u4"), ("flags", "<u4"), ("query_reversed", "<u4"), ("n_anchors", "<u4"),
                     ("n_matches", "<i4"), ("n_mismatches", "<i4"), ("n_deletions", "<i4"), ("n_insertions", "<i4"),
                     ("overhang_start", "<u4"), ("overhang_end", "<u4"), ("align_length", "<u4"), ("n_seeds", "<u4"),
                     ("reference_start", "<u4"), ("reference_end", "<u4"), ("query_start", "<u4"), ("query_end", "<u4")])
SUMMARY_FIELDS = ("query_reversed", "n_matches", "n_mismatches", "n_deletions", "n_insertions", "overhang_start", "overhang_end", "align_length",
                  "reference_start", "reference_end", "query_start", "query_end")
DEFAULTS = dict(band=62, max_overhang=1000, min_overlap_length=1000, min_identity=0.96, minimizer_size=15)

FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "read_verify")


def fixture_manifest() -> dict:
    with open(os.path.join(FIXTURE_DIR, "manifest.json")) as f:
        return json.load(f)


def load_fixture(name: str) -> dict:
    """tests/golden/read_verify/<name>.npz with its delta-coded arrays summed up again."""
    delta = set(fixture_manifest()["delta_coded"])
    with np.load(os.path.join(FIXTURE_DIR, name + ".npz")) as z:
        return {k: (np.cumsum(z[k].astype(np.int64)).astype(np.uint32) if k in delta else z[k]) for k in z.files}


def fixture_params(cfg: dict) -> dict:
    return {k: cfg[k] for k in DEFAULTS}


# ---- the identity and its table ------------------------------------------------------------------------------------------------------------
def identity(n_matches: int, n_seeds: int, minimizer_size: int) -> np.float32:
    """_identity (:614-630, :655): nbSeeds a long double, the divergence a float, the identity a float again."""
    seeds = np.longdouble(n_seeds)
    if np.longdouble(n_matches) == seeds:
        divergence = np.float32(0)
    elif n_matches == 0:
        divergence = np.float32(1)
    else:
        divergence = np.float32(np.longdouble(1.0) - np.power(np.longdouble(n_matches) / seeds, np.longdouble(1.0 / minimizer_size)))
    return np.float32(1.0 - np.float64(divergence))


def min_matches(n_seeds_max: int, min_identity: float, minimizer_size: int) -> np.ndarray:
    """min_matches[s]: the smallest m in 0 ... s whose identity is not below min_identity, or s + 1 -- by the full scan."""
    limit = np.float32(min_identity)
    out = np.zeros(n_seeds_max + 1, np.uint32)
    for s in range(n_seeds_max + 1):
        out[s] = next((m for m in range(s + 1) if not identity(m, s, minimizer_size) < limit), s + 1)
    return out


# ---- one pair ------------------------------------------------------------------------------------------------------------------------------
def pair_anchors(tm, tp, td, qm, qp, qd) -> dict:
    """One anchor for every (i, j) with target.m[i] == neighbour.m[j], in (i, j) order (:5051-5069 and the sort of :154-159)."""
    tm, qm = np.asarray(tm, np.uint32), np.asarray(qm, np.uint32)
    order = np.argsort(qm, kind="stable")
    keys = qm[order]
    lo, hi = np.searchsorted(keys, tm, "left"), np.searchsorted(keys, tm, "right")
    cnt = hi - lo
    ri = np.repeat(np.arange(len(tm), dtype=np.int64), cnt)
    start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    k = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(start, cnt)
    qi = order[np.repeat(lo, cnt) + k].astype(np.int64)
    return dict(ri=ri, qi=qi, rpos=np.asarray(tp, np.int64)[ri], qpos=np.asarray(qp, np.int64)[qi],
                rev=(np.asarray(td, np.uint8)[ri] != np.asarray(qd, np.uint8)[qi]).astype(np.uint8))


def chain_walk(rpos, qpos, rev, band, stats=None) -> list:
    """chainAnchors (:735-858) with argmaxPosition (:862-961): the best anchor's chain, root first.  band None: unlimited."""
    n = len(rpos)
    rp, qp = np.asarray(rpos, np.int64), np.asarray(qpos, np.int64)
    score = np.full(n, 20, np.int64)
    parent = np.full(n, -1, np.int64)
    for i in range(1, n):
        lo = 0 if band is None else max(0, i - band)
        j = np.arange(i - 1, lo - 1, -1)               # walked downwards, replaced on > only: the largest j wins a tie
        d_r = rp[i] - rp[j]
        d_q = qp[j] - qp[i] if rev[i] else qp[i] - qp[j]
        gap = np.abs(d_r - d_q)
        ok = (rev[j] == rev[i]) & (d_r != 0) & (d_q != 0) & (d_q <= 5000) & (d_r <= 5000) & (d_r > 0) & (gap <= 100) & (d_q >= 0)
        new = np.where(ok, score[j] + 20 - gap, 0)
        if len(new) and new.max() > 0:
            k = int(np.argmax(new))
            score[i], parent[i] = new[k], j[k]
            if stats is not None and int((new == new[k]).sum()) > 1:
                stats["pred_ties"] = stats.get("pred_ties", 0) + 1
    best = int(np.argmax(score))                       # the smallest i wins a tie (:810-815)
    if stats is not None and int((score == score[best]).sum()) > 1:
        stats["end_ties"] = stats.get("end_ties", 0) + 1
    walk = []
    at = best
    while at != -1:
        walk.append(at)
        at = int(parent[at])
    return walk[::-1]


def summary(walk, an, tp, qp, len_t, len_q) -> dict:
    """What computeChainingAlignment leaves of a chain (:274-307, :356-428, :547-569, :581-582, :614, :657-673)."""
    n_t, n_q = len(tp), len(qp)
    ri, qi = an["ri"], an["qi"]
    f, l = walk[0], walk[-1]
    fr, fq, lr, lq = int(ri[f]), int(qi[f]), int(ri[l]), int(qi[l])
    assert lr >= 3 and (fq >= 3 if fq > lq else lq >= 3), "a chain of 4 strictly monotone anchors"
    tp, qp = [int(x) for x in tp], [int(x) for x in qp]
    rev = fq > lq
    if rev:
        over_start, start_mis = min(tp[fr], len_q - qp[fq - 1]), min(fr, n_q - fq - 1)
        over_end, end_mis = min(len_t - tp[lr - 1], qp[lq]), min(n_t - lr - 1, lq)
    else:
        over_start, start_mis = min(tp[fr], qp[fq]), min(fr, fq)
        over_end, end_mis = min(len_t - tp[lr - 1], len_q - qp[lq - 1]), min(n_t - lr - 1, n_q - lq - 1)
    mis = dele = ins = 0
    for a, b in zip(walk[:-1], walk[1:]):
        rg = int(ri[b]) - int(ri[a]) - 1
        qg = int(qi[a]) - int(qi[b]) - 1 if rev else int(qi[b]) - int(qi[a]) - 1
        m = min(rg, qg)
        mis += m
        if rg > qg:
            dele += rg - m
        else:
            ins += qg - m
    m = len(walk)
    n_mis = start_mis + mis + end_mis
    u32 = lambda v: v & 0xFFFFFFFF
    return dict(query_reversed=int(rev), n_matches=m, n_mismatches=n_mis, n_deletions=dele, n_insertions=ins, overhang_start=u32(over_start),
                overhang_end=u32(over_end), align_length=u32(tp[lr] - tp[fr]), n_seeds=min(m + n_mis + dele, m + n_mis + ins), reference_start=tp[fr],
                reference_end=tp[lr], query_start=qp[lq] if rev else qp[fq], query_end=qp[fq] if rev else qp[lq])


def kept(row: dict, table: np.ndarray, max_overhang: int, min_overlap_length: int) -> bool:
    """:5088-5094, the identity by table."""
    return bool(row["overhang_start"] <= max_overhang and row["overhang_end"] <= max_overhang and row["align_length"] >= min_overlap_length and
                row["n_seeds"] < len(table) and row["n_matches"] >= table[row["n_seeds"]])


# ---- a whole call --------------------------------------------------------------------------------------------------------------------------
def verify(sel_offsets, sel_neighbour, reads: dict, target_first_read=0, reads_first_read=0, band=62, max_overhang=1000, min_overlap_length=1000, min_identity=0.96,
           minimizer_size=15, stats=None) -> dict:
    """reads: dict(offsets, minimizers, positions, directions, lengths).  Returns what capi.Verification.to_host() returns."""
    off = np.asarray(reads["offsets"], np.int64)
    n_reads = len(off) - 1
    so = np.asarray(sel_offsets, np.int64)
    rows = np.zeros(int(so[-1]), VERIFIED)
    rows["neighbour"] = np.asarray(sel_neighbour, np.uint32)
    longest = int(np.diff(off).max()) if n_reads else 0
    table = min_matches(longest, min_identity, minimizer_size)
    piece = lambda k, r: reads[k][off[r]:off[r + 1]]
    for t in range(len(so) - 1):
        tl = target_first_read + t - reads_first_read
        for s in range(int(so[t]), int(so[t + 1])):
            ql = int(rows["neighbour"][s]) - reads_first_read
            if not (0 <= tl < n_reads and 0 <= ql < n_reads):
                rows["flags"][s] = VERIFY_ABSENT
                continue
            an = pair_anchors(piece("minimizers", tl), piece("positions", tl), piece("directions", tl), piece("minimizers", ql), piece("positions", ql), piece("directions", ql))
            n = len(an["ri"])
            if n >= TOO_LONG_FROM:
                rows["flags"][s] = VERIFY_TOO_LONG
                continue
            rows["n_anchors"][s] = n
            if n < MIN_ANCHORS:
                continue
            walk = chain_walk(an["rpos"], an["qpos"], an["rev"], band, stats)
            if len(walk) < MIN_CHAIN:
                continue
            row = summary(walk, an, piece("positions", tl), piece("positions", ql), int(reads["lengths"][tl]), int(reads["lengths"][ql]))
            for k, v in row.items():
                rows[k][s] = v
            rows["flags"][s] = VERIFY_CHAIN | (VERIFY_KEPT if kept(row, table, max_overhang, min_overlap_length) else 0)
    return with_kept_lists(so, rows)


def with_kept_lists(row_offsets, rows) -> dict:
    so = np.asarray(row_offsets, np.int64)
    keep = (rows["flags"] & VERIFY_KEPT) != 0
    kpos = np.concatenate([[0], np.cumsum(keep)])
    return dict(row_offsets=so.astype(np.uint64), rows=rows, kept_offsets=kpos[so].astype(np.uint64), kept_neighbour=rows["neighbour"][keep].astype(np.uint32),
                kept_reversed=rows["query_reversed"][keep].astype(np.uint8))


def fixture_reads(d: dict) -> dict:
    return dict(offsets=d["read_offsets"], minimizers=d["minimizers"], positions=d["positions"], directions=d["directions"], lengths=d["read_lengths"])


def fixture_verification(d: dict) -> dict:
    """The REFERENCE's rows of a fixture file in the layout of capi.Verification.to_host() (n_seeds from its own counts, :581-582 + :614)."""
    rows = np.zeros(len(d["sel_neighbour"]), VERIFIED)
    rows["neighbour"] = d["sel_neighbour"]
    rows["n_anchors"] = d["row_n_anchors"]
    chain = d["row_chain"] != 0
    for k in SUMMARY_FIELDS:
        rows[k] = d["row_" + k]
    m, mis = d["row_n_matches"].astype(np.int64), d["row_n_mismatches"].astype(np.int64)
    rows["n_seeds"] = np.where(chain, np.minimum(m + mis + d["row_n_deletions"], m + mis + d["row_n_insertions"]), 0)
    rows["flags"] = np.where(chain, VERIFY_CHAIN, 0) | np.where(d["row_kept"] != 0, VERIFY_KEPT, 0)
    return with_kept_lists(d["sel_offsets"], rows)


def info(v: dict) -> dict:
    return dict(n_targets=len(v["row_offsets"]) - 1, n_rows=len(v["rows"]), n_chains=int(((v["rows"]["flags"] & VERIFY_CHAIN) != 0).sum()), n_kept=len(v["kept_neighbour"]))


def same(a: dict, b: dict) -> None:
    assert sorted(a) == sorted(b)
    for k in ("row_offsets", "kept_offsets", "kept_neighbour", "kept_reversed"):
        assert np.array_equal(a[k], b[k]), k
    for f in VERIFIED.names:
        bad = np.flatnonzero(a["rows"][f] != b["rows"][f])
        assert len(bad) == 0, (f, bad[:5], a["rows"][bad[:5]], b["rows"][bad[:5]])
