"""A numpy restatement of what mdbg_spans_extract / mdbg_reads_extract_ranges return, for tests/test_gpu_kminmer_sequences.py: the range a
(window, part) request names (ToBasespaceGfa::extractKminmerSequence, toBasespace/ToBasespaceGfa.hpp:1050-1103), the oriented string
(memcpy + Utils::revcomp) as far as the packed reads still know it, and its two forms -- the characters, and DnaBitset2's bytes
(utils/DnaBitset.hpp:118-242) -- laid out with every sequence at a multiple of 8 bytes and zero padding.
tests/test_kminmer_sequences_model.py compares it with the reference's answers under tests/golden/kminmer_sequences."""
from __future__ import annotations

import numpy as np

ENTIRE, LEFT, RIGHT = 0, 1, 2
BITSET, ASCII = 0, 1

# what the packed read keeps of a character: N under bit 3 (the invalid mask), else the upper-case base of its 2-bit code (c >> 1) & 3
KNOWN = bytes(ord("N") if c & 8 else b"ACTG"[(c >> 1) & 3] for c in range(256))
COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")
_CODE = np.zeros(256, np.uint8)                   # DnaBitset2's switch: A 0, C 1, G 2, T 3, anything else leaves the bits 0
_CODE[ord("C")], _CODE[ord("G")], _CODE[ord("T")] = 1, 2, 3


def part_range(ps, pe, ls, le, rev, part):
    """(start, length) of the read's range per request; all arguments arrays of one length.  The reference keeps the first ls / last le
    characters of the ORIENTED string: for a reversed window those are the range's far / near end."""
    ps, pe, ls, le = (np.asarray(a, dtype=np.int64) for a in (ps, pe, ls, le))
    rev, part = np.asarray(rev) != 0, np.asarray(part)
    start = np.where(part == ENTIRE, ps, np.where(part == LEFT, np.where(rev, pe - ls, ps), np.where(rev, ps, pe - le)))
    length = np.where(part == ENTIRE, pe - ps, np.where(part == LEFT, ls, le))
    return start, length


def oriented(seq: bytes, start: int, length: int, reversed_: bool) -> bytes:
    s = seq[start:start + length].translate(KNOWN)
    return s[::-1].translate(COMPLEMENT) if reversed_ else s


def bitset(s: bytes) -> np.ndarray:
    """DnaBitset2::_m_data of a string: base i in byte i / 4 at bits 6 - 2 (i % 4)."""
    c = _CODE[np.frombuffer(s, dtype=np.uint8)]
    c = np.concatenate([c, np.zeros(-len(c) % 4, np.uint8)]).reshape(-1, 4)
    return (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8)


def window_read(window_offsets, windows) -> np.ndarray:
    """The read of every flat window index."""
    return np.searchsorted(np.asarray(window_offsets, dtype=np.uint64), np.asarray(windows, dtype=np.uint64), side="right") - 1


def expected(seqs: list[bytes], read, start, length, reversed_, form: int) -> dict:
    """byte_offsets / lengths / bytes as mdbg_sequences_to_host returns them."""
    parts = []
    for r, s, n, v in zip(read, start, length, reversed_):
        o = oriented(seqs[int(r)], int(s), int(n), bool(v))
        parts.append(np.frombuffer(o, dtype=np.uint8) if form == ASCII else bitset(o))
    sizes = np.array([len(p) for p in parts], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum((sizes + 7) // 8 * 8)]).astype(np.uint64)
    out = np.zeros(int(off[-1]), np.uint8)
    for p, o in zip(parts, off[:-1]):
        out[int(o):int(o) + len(p)] = p
    return dict(byte_offsets=off, lengths=np.asarray(length, dtype=np.uint32), bytes=out)


def expected_requests(seqs: list[bytes], spans: dict, windows, parts, form: int) -> dict:
    """... for (window, part) requests over the host copy of the spans (mdbg_spans_to_host)."""
    w = np.asarray(windows, dtype=np.int64)
    rev = spans["reversed"][w]
    start, length = part_range(spans["pos_start"][w], spans["pos_end"][w], spans["seq_length_start"][w], spans["seq_length_end"][w], rev, parts)
    return expected(seqs, window_read(spans["window_offsets"], w), start, length, rev, form)


def assert_equal(got: dict, want: dict, what: str = "") -> None:
    for f in ("byte_offsets", "lengths", "bytes"):
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {f}: {g.shape} {g.dtype} against {w.shape} {w.dtype}"
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0])
            raise AssertionError(f"{what}: {f} differs first at {at}: {g[at]} against {w[at]} ({int((g != w).sum())} of {len(g)})")


def unpadded(got: dict, form: int) -> np.ndarray:
    """The meaningful bytes of every sequence, concatenated (the fixture's layout); asserts the padding is zero."""
    off, n = got["byte_offsets"].astype(np.int64), got["lengths"].astype(np.int64)
    size = n if form == ASCII else (n + 3) // 4
    assert (off % 8 == 0).all() and np.array_equal(np.diff(off), (size + 7) // 8 * 8)
    keep = np.zeros(len(got["bytes"]), bool)
    idx = np.repeat(off[:-1] - np.concatenate([[0], np.cumsum(size)[:-1]]), size) + np.arange(int(size.sum()))
    keep[idx] = True
    assert not got["bytes"][~keep].any(), "padding is not zero"
    return got["bytes"][keep]
