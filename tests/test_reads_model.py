"""tests/reads_model.py against the reference's semantics (no GPU), and the proof that the scan's seam sweep is not vacuous.

EncoderRLE compares characters (Commons.hpp:4177-4178): a homopolymer run starts at base i exactly when c[i] != c[i-1].  The device keeps
no characters, only the code, the invalid bit and the break bit -- so the three together must say the same: code change OR invalid-bit
change OR break bit.  The oracle's run-length encoder (oracle/mdbg_oracle.c: orc_hpc_encode) gives the run starts a second time."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import reads_model as M


def _run_starts_by_the_oracle(s: bytes) -> np.ndarray:
    from oracle import pyoracle
    lib = pyoracle.lib()
    lib.orc_hpc_encode.restype = C.c_size_t
    rle = C.create_string_buffer(len(s) + 2)
    pos = (C.c_uint64 * (len(s) + 2))()
    n = lib.orc_hpc_encode(s, C.c_size_t(len(s)), 1, rle, pos)
    return np.array(pos[:n], dtype=np.int64)


def test_layout_and_bits_of_a_hand_made_batch():
    seqs = [b"", b"A", b"ACGTN", b"C" * 31 + b"aA" + b"G" * 32, b"T" * 64]
    d = M.pack(seqs)
    assert d["word_offsets"].tolist() == [0, 0, 2, 4, 8, 10] and d["lengths"].tolist() == [0, 1, 5, 65, 64]
    assert d["words"][2] == (0 | 1 << 2 | 3 << 4 | 2 << 6 | 3 << 8) and d["words"][3] == 0            # A C G T N: codes 0 1 3 2 3
    assert d["invalid"].tolist() == [0, 0, 1 << 4, 0, 0, 0, 0, 0, 0, 0]
    assert d["breaks"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0]              # "aA": a changes the code after C, A breaks at bit 0 of word 1
    assert d["words"][6] == 3 and d["words"][7] == 0                           # base 64 (G) alone in word 2; the padding word
    assert d["words"][8] == d["words"][9] == 0xAAAAAAAAAAAAAAAA
    assert d["masked"].tolist() == [0, 0, 1, 1, 0] and d["masked_list"].tolist() == [2, 3]
    assert d["has_invalid"] and d["has_break"] and d["n_masked"] == 2 and d["n_words"] == 10
    lower = M.pack([b"acgt", b"ACGT"])
    assert not lower["has_invalid"] and not lower["has_break"] and not lower["masked"].any()           # lower case alone: no bit at all ...
    lower = M.pack([b"aAcg", b"ACGT"])
    assert lower["has_invalid"] and lower["has_break"] and not lower["invalid"].any()                  # ... until a case flip inside a run
    only_n = M.pack([b"ACNNNNGT"])
    assert only_n["has_invalid"] and not only_n["has_break"]
    plain = M.pack([b"ACGT" * 40])
    assert not plain["has_invalid"] and not plain["has_break"] and plain["n_masked"] == 0 and not plain["masked"].any()


def test_marking_some_reads():
    seqs = [b"ACGT", b"ACNT", b"AaCC", b"GGGG", b"TTTn"]
    d = M.mark(seqs, [1, 3, 4])
    full = M.pack(seqs)
    assert d["masked"].tolist() == [0, 1, 0, 0, 1] and d["masked_list"].tolist() == [1, 4]
    assert d["invalid"].tolist() == [0, 0, 4, 0, 0, 0, 0, 0, 8, 0] and not d["breaks"].any() and d["has_invalid"] and not d["has_break"]
    assert np.array_equal(d["words"], full["words"]) and full["breaks"][4] == 2
    none = M.mark(seqs, [0, 3])
    assert not none["has_invalid"] and not none["has_break"] and none["n_masked"] == 0 and not none["invalid"].any()


def test_all_pairs_holds_every_ordered_pair():
    s = M.all_pairs()
    assert len(s) == 257 and set(s) == set(M.ALPHABET)
    assert len({(s[i], s[i + 1]) for i in range(256)}) == 256


def test_run_starts_are_code_change_or_invalid_change_or_break_bit():
    rng = np.random.default_rng(3)
    alphabet = np.frombuffer(M.ALPHABET, np.uint8)
    seqs = [M.all_pairs()] + [alphabet[rng.integers(0, 16, int(n))].tobytes() for n in (1, 2, 31, 32, 33, 64, 65, 200, 2049, 4097)]
    seqs += [alphabet[rng.integers(0, 16, 300) // 5 * 5 % 16].tobytes(), np.repeat(alphabet[rng.integers(0, 16, 90)], 3).tobytes()]      # long runs too
    d = M.pack(seqs)
    for r, s in enumerate(seqs):
        c = np.frombuffer(s, np.uint8)
        want = np.flatnonzero(np.concatenate([[True], c[1:] != c[:-1]]))
        code, inv, brk = M.bits_of_read(d, r)
        got = np.flatnonzero(np.concatenate([[True], (code[1:] != code[:-1]) | (inv[1:] != inv[:-1]) | (brk[1:] != 0)]))
        assert np.array_equal(got, want), r
        assert brk[0] == 0 and np.array_equal(_run_starts_by_the_oracle(s), want), r
        # and a break bit is set only where the code and the invalid bit do NOT change: the three never say the same thing twice
        assert not (brk[1:] & ((code[1:] != code[:-1]) | (inv[1:] != inv[:-1]))).any(), r
    # every bit at or past a read's end is zero, the padding word included
    for r, s in enumerate(seqs):
        w0, w1, L = int(d["word_offsets"][r]), int(d["word_offsets"][r + 1]), len(s)
        assert w1 - w0 == 2 * ((L + 63) // 64)
        for w in range(w0, w1):
            n_valid = min(max(L - 32 * (w - w0), 0), 32)
            assert int(d["words"][w]) >> (2 * n_valid) == 0 and int(d["invalid"][w]) >> n_valid == 0 and int(d["breaks"][w]) >> n_valid == 0


def test_cleaned_copy_keeps_the_words_and_drops_the_masks():
    s = M.all_pairs()
    a, b = M.pack([s]), M.pack([M.clean(s)])
    assert np.array_equal(a["words"], b["words"]) and not b["has_invalid"] and not M.is_odd(M.clean(s)) and M.is_odd(s)


@pytest.mark.parametrize("hpc", [True, False])
@pytest.mark.parametrize("density", [1.0, 0.19])
def test_the_scan_seam_sweep_is_not_vacuous(density, hpc):
    """Every case of the sweep (tests/test_gpu_read_side_masks.py) must be able to fail: the oracle's record of the odd read is another
    than that of its cleaned copy, whose 2-bit words are the same -- a scan that ignored the mask bit would give the cleaned copy's record.
    Exempt are only the first and last base (covered by trimmed k-mers alone) and, without HPC, the break-only kinds."""
    cases = M.seam_cases(density, hpc)
    assert len(cases) == len(M.SEAM_POSITIONS) * len(M.SEAM_KINDS)
    exempt = [(c["p"], c["kind"]) for c in cases if not c["differs"]]
    print(f"density {density} hpc {hpc}: {len(exempt)} of {len(cases)} cases exempt from the differs-condition: {exempt}; "
          f"most redraws {max(c['attempts'] for c in cases) - 1}")
    for c in cases:
        assert M.clean(c["seq"]) != c["seq"] and len(c["seq"]) == M.SEAM_L
        if c["judged"] and M.seam_class(c["p"]) != "end":
            assert c["differs"], (c["p"], c["kind"])
        if not c["judged"]:
            assert not c["differs"]            # a break bit without HPC changes nothing: the reason it is not judged
    for kind in M.SEAM_KINDS:
        if hpc or kind not in M.BREAK_ONLY:
            for cls in ("word", "lane", "interior"):
                assert any(c["differs"] for c in cases if c["kind"] == kind and M.seam_class(c["p"]) == cls), (kind, cls)
