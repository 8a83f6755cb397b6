"""A read batch as the device holds it, from the rule alone (numpy, no GPU): the 2-bit words, the invalid mask, the break mask, the
per-read masked flag and the ascending masked list that mdbg_reads_from_ascii, mdbg_reads_mark_ascii and mdbg_reads_from_fastx_bytes
build.  The rule, per character c of a read of L bases:

  words per read   2 * ceil(L / 64); base i sits in word i // 32 of its read, its code at bits [2 (i % 32), 2 (i % 32) + 2)
  code             (c >> 1) & 3                                              (utils/kmer/Kmer.hpp:462)
  invalid bit      bit 3 of c
  break bit        at base i > 0: c[i] != c[i-1] although ((c[i] ^ c[i-1]) & 0x0E) == 0 -- another character with the same code and
                   invalid bit, which EncoderRLE (it compares characters, Commons.hpp:4177-4178) takes for a new run; never at base 0
  past the end     every bit at or past L is zero in all three arrays, and so is the padding word

Also here: the reads of the scan's seam sweep (seam_cases), shared by the CPU test that proves the sweep is not vacuous and the GPU test
that runs it."""
from __future__ import annotations

import functools

import numpy as np

ALPHABET = b"ACGTacgtNnRYSWKM"        # both values of the invalid bit, of each code bit, and of the bits the break rule ignores


def _flat(seqs):
    n = len(seqs)
    lengths = np.array([len(s) for s in seqs], dtype=np.uint32).reshape(n)
    n_words = 2 * ((lengths.astype(np.uint64) + np.uint64(63)) // np.uint64(64))
    word_offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(n_words, out=word_offsets[1:])
    c = np.frombuffer(b"".join(bytes(s) for s in seqs), dtype=np.uint8)
    read = np.repeat(np.arange(n, dtype=np.int64), lengths)
    first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=first[1:])
    i = np.arange(len(c), dtype=np.int64) - first[read]            # the base's index inside its read
    return lengths, n_words, word_offsets, c, read, i


def pack(seqs) -> dict:
    """seqs (bytes each) -> dict(word_offsets, lengths, words, invalid, breaks, masked, masked_list, has_invalid, has_break, n_masked,
    n_words): every array of capi.Reads.packed_to_host() and every field of its info."""
    lengths, n_words, word_offsets, c, read, i = _flat(seqs)
    total = int(word_offsets[-1])
    word = word_offsets[read].astype(np.int64) + i // 32
    bit = (i % 32).astype(np.uint64)
    words = np.zeros(total, dtype=np.uint64)
    invalid = np.zeros(total, dtype=np.uint32)
    breaks = np.zeros(total, dtype=np.uint32)
    code = ((c >> 1) & 3).astype(np.uint64)
    inv = ((c >> 3) & 1).astype(np.uint32)
    prev = np.roll(c, 1)                                            # (of base 0 of a read: another read's last; i > 0 masks it)
    brk = ((i > 0) & (c != prev) & (((c ^ prev) & 0x0E) == 0)).astype(np.uint32)
    np.bitwise_or.at(words, word, code << (np.uint64(2) * bit))
    np.bitwise_or.at(invalid, word, inv << bit.astype(np.uint32))
    np.bitwise_or.at(breaks, word, brk << bit.astype(np.uint32))
    masked = np.zeros(len(lengths), dtype=np.uint8)
    masked[read[(inv | brk) != 0]] = 1
    return _finish(dict(word_offsets=word_offsets, lengths=lengths, words=words, invalid=invalid, breaks=breaks, masked=masked))


def _finish(d: dict) -> dict:
    d["masked_list"] = np.flatnonzero(d["masked"]).astype(np.uint32)
    d["has_break"] = bool(d["breaks"].any())
    d["has_invalid"] = bool(d["invalid"].any()) or d["has_break"]      # the library's meaning: either mask holds a bit
    d["n_masked"] = len(d["masked_list"])
    d["n_words"] = len(d["words"])
    return d


def mark(seqs, listed) -> dict:
    """A packed batch of which the reads `listed` were handed again as characters (mdbg_reads_mark_ascii): the masks of the other reads are
    zero, and the masked list holds only listed reads that carry a bit."""
    d = pack(seqs)
    n = len(d["lengths"])
    keep = np.zeros(n, dtype=bool)
    keep[np.asarray(listed, dtype=np.int64)] = True
    owner = np.repeat(np.arange(n), np.diff(d["word_offsets"]).astype(np.int64))       # the read of every word
    d["invalid"][~keep[owner]] = 0
    d["breaks"][~keep[owner]] = 0
    d["masked"][~keep] = 0
    return _finish(d)


def bits_of_read(d: dict, r: int):
    """(code, invalid bit, break bit) of every base of read r, taken back out of the arrays."""
    w0, L = int(d["word_offsets"][r]), int(d["lengths"][r])
    i = np.arange(L)
    code = ((d["words"][w0 + i // 32] >> (2 * (i % 32)).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)
    inv = ((d["invalid"][w0 + i // 32] >> (i % 32).astype(np.uint32)) & 1).astype(np.uint8)
    brk = ((d["breaks"][w0 + i // 32] >> (i % 32).astype(np.uint32)) & 1).astype(np.uint8)
    return code, inv, brk


def is_odd(s: bytes) -> bool:
    """The read holds something else than upper-case A, C, G, T (what a feeder lists for mdbg_reads_mark_ascii)."""
    return bool(bytes(s).translate(None, b"ACGT"))


def clean(s: bytes) -> bytes:
    """The plain read with the same 2-bit words: every character replaced by the upper-case base of its code."""
    return bytes(np.frombuffer(b"ACTG", np.uint8)[(np.frombuffer(bytes(s), np.uint8) >> 1) & 3])


def all_pairs() -> bytes:
    """257 characters of ALPHABET in which every one of the 256 ordered pairs of neighbours occurs: an Euler circuit of the complete
    directed graph with loops on 16 nodes (Hierholzer), closed by its first character."""
    k = len(ALPHABET)
    nxt = [0] * k                          # edges a -> 0, 1, ... k-1 of every node, taken in order
    stack, circuit = [0], []
    while stack:
        a = stack[-1]
        if nxt[a] < k:
            stack.append(nxt[a])
            nxt[a] += 1
        else:
            circuit.append(stack.pop())
    s = bytes(ALPHABET[a] for a in reversed(circuit))
    assert len(s) == k * k + 1
    return s


# ---- the scan's seam sweep: reads of SEAM_L random bases with one odd spot at base p -------------------------------------------------
SEAM_K, SEAM_L = 15, 2300
SEAM_POSITIONS = (0, 1, SEAM_K - 1, SEAM_K, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, SEAM_L - SEAM_K - 1, SEAM_L - SEAM_K, SEAM_L - 2, SEAM_L - 1)
SEAM_KINDS = ("N", "K", "lower", "R")         # invalid bit; invalid bit and a code; break bit that splits a run; break bit, same code
BREAK_ONLY = ("lower", "R")                    # these change the homopolymer runs and nothing else: judged with HPC on only
SEAM_SEED = 20240
MAX_REDRAWS = 400


def seam_class(p: int) -> str:
    """word: a 32-base word border; lane: base 2048, word 64 of a read, a lane's second trip; end: the first and the last base, which
    only the two k-mers the parser trims (its _trimBps = 1, one k-mer at either end) cover; interior: the rest."""
    if p in (31, 32, 33, 63, 64, 65):
        return "word"
    if p in (2047, 2048, 2049):
        return "lane"
    return "end" if p in (0, SEAM_L - 1) else "interior"


def seam_read(case: int, p: int, kind: str, attempt: int) -> bytes:
    rng = np.random.default_rng([SEAM_SEED, case, attempt])
    s = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, SEAM_L)].tobytes())
    run = min(max(p - 1, 0), SEAM_L - 3)           # a run of three around p for the two kinds that sit inside one
    if kind == "N":
        s[p] = ord("N")
    elif kind == "K":
        s[p] = ord("K")
    elif kind == "lower":
        s[run:run + 3] = bytes([s[p]]) * 3
        s[p] = s[p] + 32
    else:
        s[run:run + 3] = b"CCC"
        s[p] = ord("R")
    return bytes(s)


@functools.lru_cache(maxsize=None)
def seam_cases(density: float, hpc: bool) -> tuple:
    """Every (position, kind) as dict(p, kind, seq, judged, differs, attempts): `differs` says whether the oracle's record of the read is
    another than that of its cleaned copy, which alone makes the case able to catch a mask bit the scan ignores.  At density 1.0 every
    k-mer is visible and the body is drawn once.  Below, an interior case is redrawn from its fixed seed until it differs.  Break-only
    kinds without HPC (they change nothing there) and the end positions are drawn once and stay in the sweep as they come."""
    from oracle import pyoracle as orc

    def differs(s):
        return orc.read_selection(s, None, K=SEAM_K, density=density, hpc=hpc)["record"] != \
            orc.read_selection(clean(s), None, K=SEAM_K, density=density, hpc=hpc)["record"]

    out = []
    for case, (p, kind) in enumerate((p, kind) for p in SEAM_POSITIONS for kind in SEAM_KINDS):
        judged = hpc or kind not in BREAK_ONLY
        redraw = judged and density < 1.0 and seam_class(p) != "end"
        for attempt in range(MAX_REDRAWS if redraw else 1):
            s = seam_read(case, p, kind, attempt)
            d = differs(s)
            if d:
                break
        if redraw and not d:
            raise AssertionError(f"seam case p={p} kind={kind}: no body in {MAX_REDRAWS} draws makes the oracle's record differ")
        out.append(dict(p=p, kind=kind, seq=s, judged=judged, differs=d, attempts=attempt + 1))
    return tuple(out)
