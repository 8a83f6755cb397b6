"""numpy restatement of the per-position selection (mdbg_map_select / mdbg_selection_from_host / mdbg_map_select_merge /
mdbg_selection_to_alignment_bytes), written from ReadMapper.hpp: addAlignmentScore (:1233-1313) with AlignmentScoreComparator (:90-97),
mergeAlignmentScore (:365-443), writeAlignments (:1391-1410).  ``select`` is the closed form -- per position the first `coverage` of the
candidates covering it under (score descending, read ascending) -- and ``heaps`` the reference's procedure itself, heap by heap, which
also says who was pushed and evicted again.  tests/test_read_select_model.py holds both against the reference's own output
(tests/golden/read_select); the GPU tests use the closed form on inputs the fixture does not have.  The layouts are those of
capi.Selection.to_host()."""
from __future__ import annotations

import heapq
import json
import os

import numpy as np

SELECTED = np.dtype([("ref_read", "<u4"), ("score", "<i4"), ("n_matches", "<u4"), ("part", "<u4"), ("pair", "<u8")])
CHAIN_FOUND = 1
FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "read_select")


def fixture_manifest() -> dict:
    with open(os.path.join(FIXTURE_DIR, "manifest.json")) as f:
        return json.load(f)


def load_fixture(name: str) -> dict:
    """tests/golden/read_select/<name>.npz with its delta-coded arrays summed up again."""
    delta = set(fixture_manifest()["delta_coded"])
    with np.load(os.path.join(FIXTURE_DIR, name + ".npz")) as z:
        return {k: (np.cumsum(z[k].astype(np.int64)).astype(np.uint32) if k in delta else z[k]) for k in z.files}


def list_scores(match_offsets, matches) -> np.ndarray:
    """2 n - (last - first + 1) of every (non-empty) list: mergeAlignmentScore's loop (:376-382)."""
    mo = np.asarray(match_offsets, np.int64)
    m = np.asarray(matches, np.int64)
    n = np.diff(mo)
    return (2 * n - (m[mo[1:] - 1] - m[mo[:-1]] + 1)).astype(np.int32) if len(n) else np.zeros(0, np.int32)


def candidates(cand_offsets, ref_read, score, match_offsets, matches, part=None, pair=None) -> dict:
    """The view the selection reads: per query (cand_offsets) the candidates in ascending ref_read, per candidate score and match list."""
    n = len(ref_read)
    return dict(cand_offsets=np.asarray(cand_offsets, np.uint64), ref_read=np.asarray(ref_read, np.uint32), score=np.asarray(score, np.int32),
                match_offsets=np.asarray(match_offsets, np.uint64), matches=np.asarray(matches, np.uint32),
                part=np.zeros(n, np.uint32) if part is None else np.asarray(part, np.uint32), pair=np.arange(n, dtype=np.uint64) if pair is None else np.asarray(pair, np.uint64))


def from_chains(ch: dict) -> dict:
    """The candidates of a Chains.to_host(): the rows with flags == MDBG_CHAIN_FOUND, score = alignment_score, pair = the row's index."""
    rows = ch["chains"]
    take = np.flatnonzero(rows["flags"] == CHAIN_FOUND)
    po = ch["pair_offsets"].astype(np.int64)
    before = np.concatenate([[0], np.cumsum(rows["flags"] == CHAIN_FOUND)])
    mo = ch["match_offsets"].astype(np.int64)
    lens = np.diff(mo)[take]
    new_mo = np.concatenate([[0], np.cumsum(lens)])
    idx = np.repeat(mo[take] - new_mo[:-1], lens) + np.arange(new_mo[-1])
    return candidates(before[po], rows["ref_read"][take], rows["alignment_score"][take], new_mo, ch["matches"][idx], pair=take)


def from_lists(sel_offsets, ref_read, match_offsets, matches) -> dict:
    """The candidates of stored parts (mdbg_selection_from_host): the score is computed from the list."""
    return candidates(sel_offsets, ref_read, list_scores(match_offsets, matches), match_offsets, matches)


def position_ranks(c: dict):
    """Per list element: (candidate, rank of the candidate among those covering the element's position of its query, 0 = best)."""
    co = c["cand_offsets"].astype(np.int64)
    mo = c["match_offsets"].astype(np.int64)
    n = len(c["ref_read"])
    query = np.repeat(np.arange(len(co) - 1), np.diff(co))
    cand = np.repeat(np.arange(n), np.diff(mo))
    pos = c["matches"].astype(np.int64)
    order = np.lexsort((cand, -c["score"].astype(np.int64)[cand], pos, query[cand]))       # (query, position, score descending, candidate = read ascending)
    q, p = query[cand][order], pos[order]
    head = np.concatenate([[True], (q[1:] != q[:-1]) | (p[1:] != p[:-1])]) if len(order) else np.zeros(0, bool)
    start = np.maximum.accumulate(np.where(head, np.arange(len(order)), 0)) if len(order) else np.zeros(0, np.int64)
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order)) - start
    return cand, rank


def marks(c: dict, coverage: int) -> np.ndarray:
    cand, rank = position_ranks(c)
    m = np.zeros(len(c["ref_read"]), bool)
    m[cand[rank < coverage]] = True
    return m


def compact(c: dict, m: np.ndarray) -> dict:
    """The selection of the marked candidates, in the layout of capi.Selection.to_host()."""
    co = c["cand_offsets"].astype(np.int64)
    mo = c["match_offsets"].astype(np.int64)
    take = np.flatnonzero(m)
    rows = np.zeros(len(take), SELECTED)
    rows["ref_read"], rows["score"], rows["part"], rows["pair"] = c["ref_read"][take], c["score"][take], c["part"][take], c["pair"][take]
    lens = np.diff(mo)[take]
    rows["n_matches"] = lens
    new_mo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.repeat(mo[take] - new_mo[:-1], lens) + np.arange(new_mo[-1])
    before = np.concatenate([[0], np.cumsum(m)])
    return dict(sel_offsets=before[co].astype(np.uint64), rows=rows, match_offsets=new_mo.astype(np.uint64), matches=c["matches"][idx].astype(np.uint32))


def select(c: dict, coverage: int) -> dict:
    return compact(c, marks(c, coverage))


def as_candidates(sel: dict, part: int = 0) -> dict:
    r = sel["rows"]
    return candidates(sel["sel_offsets"], r["ref_read"], r["score"], sel["match_offsets"], sel["matches"], np.full(len(r), part, np.uint32), r["pair"])


def concat(parts: list) -> dict:
    """Per query the parts' rows one behind the other; part = the part's number."""
    nq = len(parts[0]["sel_offsets"]) - 1
    cs = [as_candidates(p, i) for i, p in enumerate(parts)]
    order_c, order_m, cand_off = [], [], [0]
    base_c = np.concatenate([[0], np.cumsum([len(c["ref_read"]) for c in cs])])
    for q in range(nq):
        for i, c in enumerate(cs):
            a, b = int(c["cand_offsets"][q]), int(c["cand_offsets"][q + 1])
            order_c.append(base_c[i] + np.arange(a, b))
        cand_off.append(cand_off[-1] + sum(int(c["cand_offsets"][q + 1]) - int(c["cand_offsets"][q]) for c in cs))
    order_c = np.concatenate(order_c).astype(np.int64) if order_c else np.zeros(0, np.int64)
    cat = lambda k: np.concatenate([c[k] for c in cs])[order_c]
    lens = np.concatenate([np.diff(c["match_offsets"].astype(np.int64)) for c in cs])[order_c]
    base_m = np.concatenate([[0], np.cumsum([len(c["matches"]) for c in cs])])
    starts = np.concatenate([c["match_offsets"].astype(np.int64)[:-1] + base_m[i] for i, c in enumerate(cs)])[order_c]
    new_mo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.repeat(starts - new_mo[:-1], lens) + np.arange(new_mo[-1])
    return candidates(cand_off, cat("ref_read"), cat("score"), new_mo, np.concatenate([c["matches"] for c in cs])[idx], cat("part"), cat("pair"))


def merge(parts: list, coverage: int) -> dict:
    return select(concat(parts), coverage)


def split_by_read(c: dict, bounds) -> list:
    """The candidates cut into chunks of consecutive reference reads [bounds[i], bounds[i + 1]): what a chunked run sees."""
    co = c["cand_offsets"].astype(np.int64)
    query = np.repeat(np.arange(len(co) - 1), np.diff(co))
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        keep = (c["ref_read"] >= lo) & (c["ref_read"] < hi)
        part = compact(c, keep)
        out.append(candidates(part["sel_offsets"], part["rows"]["ref_read"], part["rows"]["score"], part["match_offsets"], part["matches"], pair=part["rows"]["pair"]))
        assert np.array_equal(np.bincount(query[keep], minlength=len(co) - 1), np.diff(part["sel_offsets"].astype(np.int64)))
    return out


def alignment_bytes(sel: dict, first_read: int = 0) -> bytes:
    """writeAlignments (:1391-1410): u32 read, u32 n, u32 ref_read[n] for every query with a selected row."""
    so = sel["sel_offsets"].astype(np.int64)
    out = []
    for q in np.flatnonzero(np.diff(so) > 0):
        out.append(np.array([first_read + q, so[q + 1] - so[q]], np.uint32))
        out.append(sel["rows"]["ref_read"][so[q]:so[q + 1]].astype(np.uint32))
    return np.concatenate(out).astype("<u4").tobytes() if out else b""


def heaps(c: dict, coverage: int, stats: dict | None = None) -> np.ndarray:
    """The reference's procedure: one heap a position, candidates in the order given (ascending read).  Returns the marks.  stats counts
    "evicted_everywhere" (pushed somewhere, left in no heap) and "ties_at_the_cut" (a candidate met a top of its own score)."""
    co = c["cand_offsets"].astype(np.int64)
    mo = c["match_offsets"].astype(np.int64)
    m = np.zeros(len(c["ref_read"]), bool)
    for q in range(len(co) - 1):
        queues: dict = {}
        pushed = set()
        for k in range(co[q], co[q + 1]):
            score, read = int(c["score"][k]), int(c["ref_read"][k])
            item = (score, -read, k)                     # the heap's top: the lowest score, among equal scores the largest read
            for p in c["matches"][mo[k]:mo[k + 1]].tolist():
                h = queues.setdefault(p, [])
                if len(h) < coverage:
                    heapq.heappush(h, item); pushed.add(k)
                    continue
                worse = h[0]
                if score < worse[0]:
                    continue
                if score == worse[0]:
                    if stats is not None:
                        stats["ties_at_the_cut"] = stats.get("ties_at_the_cut", 0) + 1
                    if read > -worse[1]:
                        continue
                heapq.heapreplace(h, item); pushed.add(k)
        left = {item[2] for h in queues.values() for item in h}
        m[list(left)] = True
        if stats is not None:
            stats["evicted_everywhere"] = stats.get("evicted_everywhere", 0) + len(pushed - left)
    return m


def conditions(c: dict, coverage: int, parts: list, merged_marks_of_chunk_rows: np.ndarray) -> dict:
    """What the fixture must exercise (asserted by the generator and by tests/test_read_select_model.py): not measurements.
    parts: the per-chunk selections; merged_marks_of_chunk_rows: per row of concat(parts), whether the merge kept it."""
    cand, rank = position_ranks(c)
    co = c["cand_offsets"].astype(np.int64)
    query = np.repeat(np.arange(len(co) - 1), np.diff(co))
    pos = c["matches"].astype(np.int64)
    depth_key = query[cand] * (1 << 32) + pos
    keys, depth = np.unique(depth_key, return_counts=True)
    deep_queries = len(np.unique(keys[depth > coverage] >> 32))
    score = c["score"].astype(np.int64)[cand]
    at_cut = dict(zip(depth_key[rank == coverage - 1].tolist(), score[rank == coverage - 1].tolist()))
    ties = sum(1 for k, s in zip(depth_key[rank == coverage].tolist(), score[rank == coverage].tolist()) if at_cut.get(k) == s)
    winning = np.bincount(cand[rank < coverage], minlength=len(c["ref_read"]))
    stats: dict = {}
    hm = heaps(c, coverage, stats)
    assert np.array_equal(hm, winning > 0), "the closed form is not the heap procedure"
    out = dict(queries_with_a_position_above_coverage=int(deep_queries), positions_tied_at_the_cut=int(ties), selected_through_one_position=int((winning == 1).sum()),
               took_part_selected_nowhere=int((winning == 0).sum()), pushed_and_evicted_everywhere=int(stats.get("evicted_everywhere", 0)),
               selected_in_chunk_dropped_by_merge=int((~merged_marks_of_chunk_rows).sum()), candidates_scoring_0_or_less=int((c["score"] <= 0).sum()))
    assert out["queries_with_a_position_above_coverage"] >= 20 and out["positions_tied_at_the_cut"] >= 5 and out["selected_through_one_position"] >= 10, out
    assert out["took_part_selected_nowhere"] >= 10 and out["pushed_and_evicted_everywhere"] >= 1 and out["selected_in_chunk_dropped_by_merge"] >= 5, out
    assert out["candidates_scoring_0_or_less"] >= 1, out
    return out


def fixture_candidates(d: dict) -> dict:
    """The reference's candidates of a fixture (every group with a chain, whole set), in the layout of ``candidates``."""
    nq = len(d["read_offsets"]) - 1
    co = np.concatenate([[0], np.cumsum(np.bincount(d["cand_query"], minlength=nq))])
    return candidates(co, d["cand_ref_read"], d["cand_score"], np.concatenate([[0], np.cumsum(d["cand_n_matches"].astype(np.int64))]), d["cand_matches"])


def fixture_marks(d: dict, c: dict, name: str) -> np.ndarray:
    """Which candidates the reference selected: name = "whole", "chunk<i>" or "merged" (per query offsets and reads)."""
    so = d[name + "_offsets"].astype(np.int64)
    want = np.repeat(np.arange(len(so) - 1, dtype=np.int64), np.diff(so)) << 32 | d[name + "_ref_read"].astype(np.int64)
    co = c["cand_offsets"].astype(np.int64)
    have = np.repeat(np.arange(len(co) - 1, dtype=np.int64), np.diff(co)) << 32 | c["ref_read"].astype(np.int64)
    assert np.isin(want, have).all() and len(np.unique(want)) == len(want), name
    return np.isin(have, want)


def fixture_chunks(d: dict, c: dict) -> list:
    """The reference's per-chunk selections as selections (rows of the whole set's candidates; pair = the candidate's number)."""
    return [compact(c, fixture_marks(d, c, f"chunk{i}")) for i in range(len(d["chunk_bounds"]) - 1)]


def fixture_merged(d: dict, c: dict) -> dict:
    """The reference's merged selection in the layout ``merge`` gives: part = the chunk of the row's read."""
    sel = compact(c, fixture_marks(d, c, "merged"))
    sel["rows"]["part"] = np.searchsorted(d["chunk_bounds"].astype(np.int64), sel["rows"]["ref_read"].astype(np.int64), side="right") - 1
    return sel


def same(a: dict, b: dict) -> None:
    """Two selections in one layout are equal, array for array."""
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (k, a[k].dtype, b[k].dtype, a[k].shape, b[k].shape)
        if not np.array_equal(a[k], b[k]):
            at = int(np.flatnonzero(a[k] != b[k])[0])
            raise AssertionError(f"{k} differs first at {at}: {a[k][at]} against {b[k][at]}")
