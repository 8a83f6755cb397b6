"""A numpy restatement of what mdbg_kminmer_spans returns, for tests/test_gpu_kminmer_spans.py: EncoderRLE::execute's coordinate map over the
characters of a read (Commons.hpp:4163-4203), the spans [S, E) = [rle[p], rle[p + l]) of its minimizers, and per window of k minimizers the
ReadKminmer fields of MDBG::getKminmers (Commons.hpp:5401-5526) with the identity from the oracle (pyoracle.kminmer_normalize_hash)."""
from __future__ import annotations

import numpy as np

from oracle import pyoracle as orc

FIELDS = ("window_offsets", "min_start", "min_end", "hash_lo", "hash_hi", "reversed", "pos_start", "pos_end", "seq_length_start", "seq_length_end")


def rle_positions(seq: bytes, hpc: bool) -> np.ndarray:
    """rle[j] for j = 0 .. L' (rle[L'] = the read's length); the identity without compression."""
    c = np.frombuffer(seq, dtype=np.uint8)
    if not hpc:
        return np.arange(len(c) + 1, dtype=np.int64)
    start = np.ones(len(c), dtype=bool)
    start[1:] = c[1:] != c[:-1]            # the reference compares characters
    return np.concatenate([np.flatnonzero(start), [len(c)]]).astype(np.int64)


def expected(seqs: list[bytes], offsets, minimizers, positions, l: int, hpc: bool, k: int) -> dict:
    offsets = np.asarray(offsets, dtype=np.int64)
    mins = np.asarray(minimizers, dtype=np.uint32)
    pos = np.asarray(positions, dtype=np.int64)
    S = np.zeros(len(mins), np.uint32)
    E = np.zeros(len(mins), np.uint32)
    out = {f: [] for f in FIELDS[3:]}
    counts = []
    for r, seq in enumerate(seqs):
        a, b = int(offsets[r]), int(offsets[r + 1])
        n = b - a
        rle = rle_positions(seq, hpc)
        p = pos[a:b]
        assert (np.diff(p) > 0).all() and (n == 0 or p[-1] + l < len(rle)), "positions are not this read's"
        S[a:b], E[a:b] = rle[p], rle[p + l]
        nw = max(0, n - k + 1)
        counts.append(nw)
        if nw == 0:
            continue
        s, e, m = S[a:b].astype(np.int64), E[a:b].astype(np.int64), mins[a:b]
        i = np.arange(nw)
        rev = np.zeros(nw, np.uint8)
        lo = np.zeros(nw, np.uint64)
        hi = np.zeros(nw, np.uint64)
        for w in range(nw):
            rv, _, h, lw = orc.kminmer_normalize_hash(m[w:w + k])
            rev[w], hi[w], lo[w] = rv, h, lw
        f, bk = s[i + 1] - s[i], e[i + k - 1] - e[i + k - 2]
        out["hash_lo"].append(lo); out["hash_hi"].append(hi); out["reversed"].append(rev)
        out["pos_start"].append(s[i].astype(np.uint32)); out["pos_end"].append(e[i + k - 1].astype(np.uint32))
        out["seq_length_start"].append(np.where(rev != 0, bk, f).astype(np.uint32))
        out["seq_length_end"].append(np.where(rev != 0, f, bk).astype(np.uint32))
    dt = dict(hash_lo=np.uint64, hash_hi=np.uint64, reversed=np.uint8)
    res = {f: (np.concatenate(v) if v else np.zeros(0, dt.get(f, np.uint32))) for f, v in out.items()}
    res["window_offsets"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    res["min_start"], res["min_end"] = S, E
    return res


def assert_equal(got: dict, want: dict, what: str = "") -> None:
    for f in FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape, f"{what}: {f}: {g.shape} against {w.shape}"
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0])
            raise AssertionError(f"{what}: {f} differs first at {at}: {g[at]} against {w[at]} ({int((g != w).sum())} of {len(g)})")
