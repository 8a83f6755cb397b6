"""numpy restatement of the read-against-read mapper (mdbg_map_index_build / mdbg_map_anchors / mdbg_map_chains), written from
ReadMapper.hpp (ReadFunctor :465-505, AlignReadsLowDensityFunctor::operator() :668-756, chainAnchors / argmaxPosition :887-1230) at
k = 2.  tests/test_read_mapper_model.py holds it against the reference's own output (tests/golden/read_mapper); the GPU tests use it
on inputs the fixture does not have.  The layouts are those of capi.MapIndex / Anchors / Chains .to_host()."""
from __future__ import annotations

import json
import os

import numpy as np

MIN_QUERY_MINIMIZERS = 10
CHAIN_FOUND, CHAIN_TOO_LONG = 1, 2
CHAIN_TOO_LONG_FROM = (1 << 24) // 80
CHAIN = np.dtype([("ref_read", "<u4"), ("flags", "<u4"), ("score", "<i4"), ("n_matches", "<u4"), ("query_reversed", "<u4"), ("reserved", "<u4"),
                  ("n_diff_query", "<i8"), ("n_diff_reference", "<i8"), ("query_start", "<i8"), ("query_end", "<i8"),
                  ("reference_start", "<i8"), ("reference_end", "<i8"), ("alignment_score", "<i8")])


FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "read_mapper")


def fixture_manifest() -> dict:
    with open(os.path.join(FIXTURE_DIR, "manifest.json")) as f:
        return json.load(f)


def load_fixture(name: str) -> dict:
    """tests/golden/read_mapper/<name>.npz with its delta-coded arrays summed up again."""
    delta = set(fixture_manifest()["delta_coded"])
    with np.load(os.path.join(FIXTURE_DIR, name + ".npz")) as z:
        return {k: (np.cumsum(z[k].astype(np.int64)).astype(np.uint32) if k in delta else z[k]) for k in z.files}


def windows(mins, offsets, positions, first_read=0) -> dict:
    """Every window of two minimizers of every read, in (read, index) order."""
    mins = np.asarray(mins, np.uint64)
    pos = np.asarray(positions, np.uint64)
    off = np.asarray(offsets, np.int64)
    lens = np.diff(off)
    nwin = np.maximum(lens - 1, 0)
    read = np.repeat(np.arange(len(lens), dtype=np.int64), nwin)
    woff = np.concatenate([[0], np.cumsum(nwin)])
    index = np.arange(woff[-1], dtype=np.int64) - woff[read]
    at = off[read] + index
    a, b = mins[at], mins[at + 1]
    return dict(pair=(np.minimum(a, b) << np.uint64(32)) | np.maximum(a, b), read=(read + first_read).astype(np.uint32),
                position=((pos[at] + pos[at + 1]) // np.uint64(2)).astype(np.uint32), index=index.astype(np.uint32),
                reversed=(a >= b).astype(np.uint8), local_read=read, window_offsets=woff)


def build_index(mins, offsets, positions, first_read=0) -> dict:
    """The windows grouped by pair, a pair's entries in (read, index) order."""
    w = windows(mins, offsets, positions, first_read)
    order = np.argsort(w["pair"], kind="stable")
    ix = {k: w[k][order] for k in ("pair", "read", "position", "index", "reversed")}
    ix["window"] = order.astype(np.int64)          # the entry's window number in the chunk
    ix["distinct"], ix["run"] = np.unique(ix["pair"], return_index=True)
    ix["run"] = np.concatenate([ix["run"], [len(order)]]).astype(np.int64)
    return ix


def index_info(ix) -> dict:
    runs = np.diff(ix["run"])
    return dict(n_entries=len(ix["pair"]), n_pairs=len(ix["distinct"]), longest_run=int(runs.max()) if len(runs) else 0)


def anchors(ix, mins, offsets, positions, query_first_read=0, min_anchors=3, query_begin=0, query_end=0) -> dict:
    off = np.asarray(offsets, np.int64)
    n_reads = len(off) - 1
    if query_begin == 0 and query_end == 0:
        query_end = n_reads
    qw = windows(mins, off, positions, query_first_read)
    lens = np.diff(off)
    cols = dict(ref_read=[], ref_position=[], ref_index=[], query_position=[], query_index=[], reversed=[])
    pair_offsets, pair_ref, anchor_offsets = [0], [], [0]
    n_kept = 0
    for r in range(query_begin, query_end):
        rows = []
        if lens[r] >= MIN_QUERY_MINIMIZERS:
            w0, w1 = qw["window_offsets"][r], qw["window_offsets"][r + 1]
            k = np.searchsorted(ix["distinct"], qw["pair"][w0:w1])
            for i in range(w1 - w0):
                if k[i] >= len(ix["distinct"]) or ix["distinct"][k[i]] != qw["pair"][w0 + i]:
                    continue
                e = np.arange(ix["run"][k[i]], ix["run"][k[i] + 1])
                e = e[ix["read"][e] != query_first_read + r]
                rows.append(np.stack([ix["read"][e], ix["position"][e], ix["index"][e], np.full(len(e), qw["position"][w0 + i]), np.full(len(e), i),
                                      ix["reversed"][e] != qw["reversed"][w0 + i]], axis=1).astype(np.int64))
        rows = np.concatenate(rows) if rows else np.zeros((0, 6), np.int64)
        rows = rows[np.lexsort((rows[:, 3], rows[:, 1], rows[:, 0]))]
        heads = np.flatnonzero(np.concatenate([[True], rows[1:, 0] != rows[:-1, 0]])) if len(rows) else np.zeros(0, np.int64)
        ends = np.concatenate([heads[1:], [len(rows)]]) if len(rows) else heads
        for h, t in zip(heads, ends):
            if t - h < min_anchors:
                continue
            for c, name in enumerate(cols):
                cols[name].append(rows[h:t, c])
            pair_ref.append(rows[h, 0])
            n_kept += t - h
            anchor_offsets.append(n_kept)
        pair_offsets.append(len(pair_ref))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    out = dict(pair_offsets=np.asarray(pair_offsets, np.uint64), pair_ref_read=np.asarray(pair_ref, np.uint32), anchor_offsets=np.asarray(anchor_offsets, np.uint64))
    out.update({name: cat(cols[name], np.uint8 if name == "reversed" else np.uint32) for name in cols})
    return out


def chain_pair(rpos, qpos, rev, ridx, qidx, band, stats=None):
    """chainAnchors on one pair's anchors: (row fields or None, match list).  band None: unlimited.  stats (optional dict) counts
    "pred_ties" (anchors at which two predecessors tie for the best score) and "end_ties" (the best score reached by two anchors)."""
    n = len(rpos)
    rp, qp = np.asarray(rpos, np.int64), np.asarray(qpos, np.int64)
    rev = np.asarray(rev, np.uint8)
    score = np.full(n, 20, np.int64)
    parent = np.full(n, -1, np.int64)
    for i in range(1, n):
        lo = 0 if band is None else max(0, i - band)
        j = np.arange(i - 1, lo - 1, -1)               # the reference walks downwards and replaces on > only: the largest j wins a tie
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
    best = int(np.argmax(score))                       # the smallest i wins a tie
    if stats is not None and int((score == score[best]).sum()) > 1:
        stats["end_ties"] = stats.get("end_ties", 0) + 1
    walk = []
    at = best
    while at != -1:
        walk.append(at)
        at = int(parent[at])
    if len(walk) < 3:
        return None, []
    first, last, m = walk[0], walk[-1], len(walk)
    fq, lq = int(qidx[first]), int(qidx[last])
    u32 = lambda v: v & 0xFFFFFFFF
    qrev = fq > lq
    matches = [int(qidx[a]) for a in walk]
    if qrev:
        ndq, qs, qe = u32(fq - lq + 1) - m, lq, fq
        matches.reverse()
    else:
        ndq, qs, qe = u32(lq - fq + 1) - m, fq, lq
    row = dict(flags=CHAIN_FOUND, score=int(score[best]), n_matches=m, query_reversed=int(qrev), n_diff_query=ndq,
               n_diff_reference=u32(int(ridx[first]) - int(ridx[last]) + 1) - m, query_start=qs, query_end=qe, reference_start=int(rp[first]),
               reference_end=int(rp[last]), alignment_score=m - ndq)
    return row, matches


def chains(an, band, stats=None) -> dict:
    n_pairs = len(an["pair_ref_read"])
    rows = np.zeros(n_pairs, CHAIN)
    rows["ref_read"] = an["pair_ref_read"]
    match_offsets, matches = [0], []
    ao = an["anchor_offsets"].astype(np.int64)
    for p in range(n_pairs):
        a, b = ao[p], ao[p + 1]
        if b - a >= CHAIN_TOO_LONG_FROM:
            rows[p]["flags"] = CHAIN_TOO_LONG
        else:
            row, m = chain_pair(an["ref_position"][a:b], an["query_position"][a:b], an["reversed"][a:b], an["ref_index"][a:b], an["query_index"][a:b], band, stats)
            if row is not None:
                for k, v in row.items():
                    rows[p][k] = v
                matches.extend(m)
        match_offsets.append(len(matches))
    return dict(pair_offsets=an["pair_offsets"].copy(), chains=rows, match_offsets=np.asarray(match_offsets, np.uint64), matches=np.asarray(matches, np.uint32))


def fixture_anchors(d: dict, min_anchors: int = 1) -> dict:
    """What the REFERENCE left in a fixture, in the layout of ``anchors``: the groups of fewer than min_anchors anchors taken out."""
    pa = d["pair_anchors"].astype(np.int64)
    keep = pa >= min_anchors
    keep_anchor = np.repeat(keep, pa)
    n_reads = len(d["read_offsets"]) - 1
    out = dict(pair_offsets=np.concatenate([[0], np.cumsum(np.bincount(d["pair_query"][keep], minlength=n_reads))]).astype(np.uint64),
               pair_ref_read=d["pair_ref_read"][keep].astype(np.uint32), anchor_offsets=np.concatenate([[0], np.cumsum(pa[keep])]).astype(np.uint64))
    for name in ("ref_read", "ref_position", "ref_index", "query_position", "query_index", "reversed"):
        out[name] = d["anchor_" + name][keep_anchor].astype(np.uint8 if name == "reversed" else np.uint32)
    return out


def fixture_chains(d: dict, min_anchors: int = 1) -> dict:
    """... and in the layout of ``chains``."""
    keep = d["pair_anchors"].astype(np.int64) >= min_anchors
    found = d["pair_score"] != 0
    rows = np.zeros(len(keep), CHAIN)
    rows["ref_read"] = d["pair_ref_read"]
    rows["flags"] = np.where(found, CHAIN_FOUND, 0)
    rows["score"] = d["pair_score"]
    for name in ("n_matches", "query_reversed", "n_diff_query", "n_diff_reference", "query_start", "query_end", "reference_start", "reference_end"):
        rows[name] = d["chain_" + name]
    rows["alignment_score"] = np.where(found, d["chain_n_matches"] - d["chain_n_diff_query"], 0)
    mo = d["match_offsets"].astype(np.int64)
    lens = np.diff(mo)
    n_reads = len(d["read_offsets"]) - 1
    return dict(pair_offsets=np.concatenate([[0], np.cumsum(np.bincount(d["pair_query"][keep], minlength=n_reads))]).astype(np.uint64), chains=rows[keep],
                match_offsets=np.concatenate([[0], np.cumsum(lens[keep])]).astype(np.uint64), matches=d["matches"][np.repeat(keep, lens)].astype(np.uint32))


def same(a: dict, b: dict) -> None:
    """Two results in one layout are equal, array for array."""
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (k, a[k].dtype, b[k].dtype, a[k].shape, b[k].shape)
        if not np.array_equal(a[k], b[k]):
            at = int(np.flatnonzero(a[k] != b[k])[0])
            raise AssertionError(f"{k} differs first at {at}: {a[k][at]} against {b[k][at]}")
