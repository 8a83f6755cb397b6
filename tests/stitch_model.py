"""A numpy restatement, over tests/extract_model.py, of what mdbg_spans_stitch / mdbg_reads_stitch_ranges / mdbg_sequences_to_fasta_bytes
return: pieces -> oriented strings -> the flip -> the invalid rule -> concatenation -> both forms -> FASTA text, as
ToBasespaceGfa::CreateBaseContigsFunctor (toBasespace/ToBasespaceGfa.hpp:1479-1795) does it over the DnaBitset2 pieces it finds stored.
tests/test_contig_stitch_model.py compares it with the reference's text under tests/golden/contig_stitch."""
from __future__ import annotations

import json
import os

import numpy as np

from tests import extract_model as EM
from tests import helpers as H

FIX = os.path.join(H.GOLDEN, "contig_stitch")
SEQUENCES = os.path.join(H.GOLDEN, "kminmer_sequences")
with open(os.path.join(FIX, "manifest.json")) as _f:
    MANIFEST = json.load(_f)

NONE = 0xFFFFFFFFFFFFFFFF                        # MDBG_STITCH_NONE
PIECE = np.dtype([("window", "<u8"), ("part", "<u4"), ("flip", "<u4")])
SUFFIX = (b"l", b"c", b"c")               # flag 2 is narrowed to `bool isCircular` (:1487): "c", the "rc" branch is never reached


def load(cfg: dict):
    """Of a configuration of the fixture: its reads, its spans (the windows of tests/golden/kminmer_sequences), its contigs as lists of
    (read, window of the read, contig window reversed, present), and the committed arrays (names, flags, text ...)."""
    with open(os.path.join(SEQUENCES, "reads.txt"), "rb") as f:
        all_reads = f.read().split(b"\n")[:-1]
    reads = [all_reads[i] for i in cfg["reads"]]
    spans = dict(np.load(os.path.join(SEQUENCES, cfg["name"] + ".npz")))
    want = np.load(os.path.join(FIX, cfg["name"] + ".npz"))
    off = want["contig_offsets"].astype(np.int64)
    rows = list(zip(want["read"].tolist(), want["window"].tolist(), want["reversed"].tolist(), want["present"].tolist()))
    return reads, spans, [rows[off[c]:off[c + 1]] for c in range(len(off) - 1)], want


def revcomp(s: bytes) -> bytes:
    return s[::-1].translate(EM.COMPLEMENT)     # (N stays N)


def pieces_by_the_rule(contigs, window_offsets) -> tuple[np.ndarray, np.ndarray]:
    """contigs: per contig a list of (read, window of the read, contig window reversed, present).  Position 0 takes ENTIRE, a later one
    RIGHT when the contig's window is forward and LEFT when it is reversed; flip is the contig window's orientation; a piece that is not
    present is MDBG_STITCH_NONE -- and still a position."""
    pieces = np.zeros(sum(len(c) for c in contigs), PIECE)
    offsets = np.zeros(len(contigs) + 1, np.uint64)
    at = 0
    for c, contig in enumerate(contigs):
        for i, (read, window, rev, present) in enumerate(contig):
            pieces[at] = (int(window_offsets[read]) + window, EM.ENTIRE if i == 0 else EM.LEFT if rev else EM.RIGHT, 1 if rev else 0) if present else (NONE, 0, 0)
            at += 1
        offsets[c + 1] = at
    return pieces, offsets


def piece_string(seqs: list[bytes], spans: dict, piece, form: int) -> bytes:
    """What one (window, part, flip) piece adds to its contig."""
    w = int(piece["window"])
    if w == NONE:
        return b""
    rev = bool(spans["reversed"][w])
    start, length = EM.part_range(*(spans[f][w:w + 1] for f in ("pos_start", "pos_end", "seq_length_start", "seq_length_end")), [rev], [int(piece["part"])])
    s = EM.oriented(seqs[int(EM.window_read(spans["window_offsets"], [w])[0])], int(start[0]), int(length[0]), rev)
    if form == EM.BITSET:
        s = s.replace(b"N", b"A")               # the piece is stored as DnaBitset2: a character outside ACGT is A ...
    return revcomp(s) if piece["flip"] else s   # ... and Utils::revcomp of a reversed contig window makes it T


def contig_strings(seqs: list[bytes], spans: dict, pieces: np.ndarray, offsets, form: int) -> list[bytes]:
    off = np.asarray(offsets, dtype=np.int64)
    return [b"".join(piece_string(seqs, spans, p, form) for p in pieces[off[c]:off[c + 1]]) for c in range(len(off) - 1)]


def range_contig_strings(seqs: list[bytes], ranges, offsets) -> list[bytes]:
    """... for (read, start, length, reversed) ranges: an invalid base is N here and code 0 in the bitset (EM.bitset packs N as 0)."""
    off = np.asarray(offsets, dtype=np.int64)
    return [b"".join(EM.oriented(seqs[int(r)], int(s), int(n), bool(v)) for r, s, n, v in ranges[off[c]:off[c + 1]]) for c in range(len(off) - 1)]


def layout(strings: list[bytes], form: int) -> dict:
    """byte_offsets / lengths / bytes as mdbg_sequences_to_host returns them: every contig at a multiple of 8 bytes, padding zero."""
    parts = [np.frombuffer(s, dtype=np.uint8) if form == EM.ASCII else EM.bitset(s) for s in strings]
    sizes = np.array([len(p) for p in parts], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum((sizes + 7) // 8 * 8)]).astype(np.uint64)
    out = np.zeros(int(off[-1]), np.uint8)
    for p, o in zip(parts, off[:-1]):
        out[int(o):int(o) + len(p)] = p
    return dict(byte_offsets=off, lengths=np.array([len(s) for s in strings], dtype=np.uint32), bytes=out)


def fasta_text(strings: list[bytes], names=None, flags=None) -> bytes:
    """The bytes CreateBaseContigsFunctor hands to gzwrite; strings in BITSET spelling (DnaBitset2::to_string knows no N)."""
    out = []
    for i, s in enumerate(strings):
        name = i if names is None else int(names[i])
        s = s.replace(b"N", b"A")
        out.append(b">ctg%dl\nA\n" % name if not s else b">ctg%d%s\n%s\n" % (name, SUFFIX[0 if flags is None else int(flags[i])], s))
    return b"".join(out)
